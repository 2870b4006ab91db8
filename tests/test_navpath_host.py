"""Paths and look-ahead waypoints on the distance fields (`ms_nav_waypoints` / `ms_nav_paths`, `DistanceFields.waypoints` /
`.paths`, `modules.PathFollower`, `PointGoal.expert`) on the CPU: the contract of include/megastep_hip.h (MsNavWaypoints)
restated in binary32 numpy (`path_rule`, which tests/test_gpu_navpath.py holds the kernels to, bit for bit); what the rule
promises - a chain that ends on the goal wherever the query is finite, no segment to a waypoint through a wall, a walker that
arrives and walks no further than the query says; the host instantiations of the kernels' own device functions against the
rule; and the C-ABI's declarations, layouts and refusals."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests.test_abi import ROOT, declared_symbols
from tests.test_navfield_host import CELL, CELLS, DIAGONAL, F, INF, RADIUS, _crossings, _world, bits, nav_rule, plans, spawn_points

NAN = F(np.nan)
NEIGHBOURS = ((0, 1), (1, 0), (0, -1), (-1, 0), (1, 1), (1, -1), (-1, -1), (-1, 1))


class path_rule:
    """The contract in numpy: every operation one binary32 operation, in the order the header gives. A `world` is what the rule
    reads of one env and one goal: (geom, cell, free (ny, nx) bool, D (ny, nx) float32, q (2,) float32)."""

    @staticmethod
    def corner(p, geom, cell):
        """(i0, j0) of point p, None without one."""
        jx0, iy0, nx, ny = geom
        c = F(cell)
        with np.errstate(all='ignore'):
            fx, fy = np.floor(F(p[0])/c - F(.5)), np.floor(F(p[1])/c - F(.5))
        if not (abs(fx) < 2.**30 and abs(fy) < 2.**30):
            return None
        return int(fy) - iy0, int(fx) - jx0

    @staticmethod
    def centre(geom, cell, i, j):
        jx0, iy0, nx, ny = geom
        return (F(jx0 + j) + F(.5))*F(cell), (F(iy0 + i) + F(.5))*F(cell)

    @staticmethod
    def leg(p, geom, cell, i, j):
        x, y = path_rule.centre(geom, cell, i, j)
        dx, dy = F(p[0]) - x, F(p[1]) - y
        return np.sqrt(dx*dx + dy*dy)

    @staticmethod
    def start(world, p):
        """(i, j, leg) of a*, None without a path."""
        geom, cell, free, D, q = world
        ny, nx = D.shape
        corner = path_rule.corner(p, geom, cell)
        if corner is None:
            return None
        best, found = INF, None
        for t in range(4):
            i, j = corner[0] + (t >> 1), corner[1] + (t & 1)
            if 0 <= i < ny and 0 <= j < nx and D[i, j] < INF:
                leg = path_rule.leg(p, geom, cell, i, j)
                s = D[i, j] + leg
                if s < best:
                    best, found = s, (i, j, leg)
        return found

    @staticmethod
    def hops(world):
        """Every cell's hop at once, as a fold over the eight shifted grids in the rule's order. Returns (kind, step, least):
        kind (ny, nx) int8 - 0 the chain ends here (next and last point q), 1 on to neighbour `step`, -1 broken; least: the
        least neighbour value."""
        geom, cell, free, D, q = world
        ny, nx = D.shape
        pf = np.zeros((ny + 2, nx + 2), bool); pf[1:-1, 1:-1] = free
        pd = np.full((ny + 2, nx + 2), INF, F); pd[1:-1, 1:-1] = D
        best, below = np.full((ny, nx), INF, F), np.full((ny, nx), INF, F)
        step = np.full((ny, nx), -1, np.int8)
        for t, (di, dj) in enumerate(NEIGHBOURS):
            ok = pf[1 + di:ny + 1 + di, 1 + dj:nx + 1 + dj]
            if di and dj:
                ok = ok & pf[1 + di:ny + 1 + di, 1:nx + 1] & pf[1:ny + 1, 1 + dj:nx + 1 + dj]
            du = pd[1 + di:ny + 1 + di, 1 + dj:nx + 1 + dj]
            w = F(cell)*DIAGONAL if di and dj else F(cell)
            with np.errstate(all='ignore'):
                v = np.where(ok, du + w, INF)
                take = v < best
            best, below, step = np.where(take, v, best), np.where(take, du, below), np.where(take, np.int8(t), step)
        with np.errstate(all='ignore'):
            kind = np.where((step >= 0) & (below < D), 1, -1).astype(np.int8)
        corner = path_rule.corner(q, geom, cell)
        if corner is not None:
            for t in range(4):
                i, j = corner[0] + (t >> 1), corner[1] + (t & 1)
                if 0 <= i < ny and 0 <= j < nx and path_rule.leg(q, geom, cell, i, j) == D[i, j]:
                    kind[i, j] = 0
        return kind, step, best

    @staticmethod
    def chain(world, p, limit=None, table=None):
        """(points [(x, y)], ended, leg(p, x_0), cells [(i, j)]) - the chain's first `limit` points (all of them: None); ended:
        its last point is q.  None without a path."""
        geom, cell, free, D, q = world
        kind, step, _ = table if table is not None else path_rule.hops(world)
        first = path_rule.start(world, p)
        if first is None:
            return None
        i, j, leg0 = first
        points, cells, ended = [], [], False
        while True:
            points.append(path_rule.centre(geom, cell, i, j)); cells.append((i, j))
            if limit is not None and len(points) >= limit:
                break
            assert len(cells) <= D.size                                  # (D falls at every hop)
            if kind[i, j] == 0:
                points.append((F(q[0]), F(q[1]))); ended = True
            if kind[i, j] != 1:
                break
            di, dj = NEIGHBOURS[step[i, j]]
            i, j = i + di, j + dj
        return points, ended, leg0, cells

    @staticmethod
    def sights(world, p, xs, ys):
        """sight(p, x) for each of the points (xs, ys), float32 arrays: (n,) bool."""
        geom, cell, free, D, q = world
        jx0, iy0, nx, ny = geom
        c, px, py = F(cell), F(p[0]), F(p[1])
        pad = np.zeros((ny + 4, nx + 4), bool); pad[2:-2, 2:-2] = free
        with np.errstate(all='ignore'):
            dx, dy = xs - px, ys - py
            k = np.ceil(np.sqrt(dx*dx + dy*dy)/(F(.5)*c))
            seen = k < 2.**20
            K = np.where(seen, k, 0).astype(np.int64)
            n = np.maximum(K - 1, 0)
            which = np.repeat(np.arange(len(xs)), n)
            s = np.arange(n.sum()) - np.repeat(np.cumsum(n) - n, n) + 1
            t = s.astype(F)/K[which].astype(F)
            x, y = px + dx[which]*t, py + dy[which]*t
            fx, fy = np.floor(x/c - F(.5)), np.floor(y/c - F(.5))
            anchored = (np.abs(fx) < 2.**30) & (np.abs(fy) < 2.**30)
            j0 = np.clip(np.where(anchored, fx, 0).astype(np.int64) - jx0, -2, nx) + 2
            i0 = np.clip(np.where(anchored, fy, 0).astype(np.int64) - iy0, -2, ny) + 2
        clear = anchored & pad[i0, j0] & pad[i0, j0 + 1] & pad[i0 + 1, j0] & pad[i0 + 1, j0 + 1]
        blocked = np.bincount(which[~clear], minlength=len(xs)) > 0
        return seen & ~blocked

    @staticmethod
    def waypoint(world, p, lookahead=16, table=None):
        """((x, y), k): the waypoint and its index; ((NaN, NaN), -1) without a path."""
        geom, cell, free, D, q = world
        found = path_rule.chain(world, p, lookahead, table)
        if found is None:
            return (NAN, NAN), -1
        points, _, leg0, _ = found
        n = len(points)
        b = 1 if leg0 <= F(.5)*F(cell) and n >= 2 else 0
        k = b
        if n - 1 > b:
            xs, ys = (np.array([pt[a] for pt in points[b + 1:]], F) for a in (0, 1))
            admissible = np.nonzero(path_rule.sights(world, p, xs, ys))[0]
            if len(admissible):
                k = b + 1 + int(admissible[-1])
        return points[k], k

    @staticmethod
    def path(world, p, max_points, table=None):
        """((max_points, 2) float32 with NaN in the slots not written, count)."""
        out = np.full((max_points, 2), NAN, F)
        found = path_rule.chain(world, p, None, table)
        if found is None:
            return out, 0
        points, ended, _, _ = found
        points = [(F(p[0]), F(p[1]))] + points
        m = min(len(points), max_points)
        out[:m] = np.array(points[:m], F)
        return out, len(points) if ended else -len(points)


# ---------------------------------------------------------------------------------------------------------------------
# the inputs: three plain and three oblique plans, a goal each, sixty starts each
# ---------------------------------------------------------------------------------------------------------------------
class _Case:
    def __init__(self, g, rng, cell=CELL, r=RADIUS):
        self.walls, self.geom, self.free = _world(g, cell, r)
        pts = spawn_points(g)
        self.goal = (pts[rng.randint(len(pts))] + rng.uniform(-.05, .05, 2)).astype(F)
        self.points = (pts[rng.choice(len(pts), 60)] + rng.uniform(-.05, .05, (60, 2))).astype(F)
        self.D = nav_rule.field(self.free, self.geom, cell, self.goal)
        self.world = (self.geom, cell, self.free, self.D, self.goal)
        self.table = path_rule.hops(self.world)
        self.g = np.array([nav_rule.query(self.D, self.geom, cell, self.free, p) for p in self.points], F)


_CASES = {}


def cases(cell=CELL, r=RADIUS):
    if (cell, r) not in _CASES:
        rng = np.random.RandomState(21)
        _CASES[cell, r] = [_Case(g, rng, cell, r) for g in plans(3) + plans(3, oblique=True)]
    return _CASES[cell, r]


def test_every_finite_query_has_a_chain_that_ends_on_the_goal():
    finite = total = longest = 0
    for case in cases():
        kind, step, least = case.table
        for p, g in zip(case.points, case.g):
            total += 1
            found = path_rule.chain(case.world, p, None, case.table)
            if not np.isfinite(g):
                assert found is None
                assert path_rule.waypoint(case.world, p, 16, case.table)[1] == -1 and path_rule.path(case.world, p, 8, case.table)[1] == 0
                continue
            finite += 1
            points, ended, leg0, cells = found
            assert ended and bits(np.array(points[-1], F)).tolist() == bits(case.goal).tolist()
            longest = max(longest, len(points))
            # at a fixed point of the relaxation the least neighbour value IS D[v], at every cell the chain leaves by a hop
            for i, j in cells[:-1]:
                assert kind[i, j] == 1 and bits(least[i, j]) == bits(case.D[i, j])
            # the path's length is the query: one rounding per addition
            path = np.array([p] + points, np.float64)
            total_length = np.linalg.norm(np.diff(path, axis=0), axis=1).sum()
            assert abs(total_length - float(g)) <= len(path)*2.**-23*max(total_length, 1.), (total_length, g)
    assert finite >= .8*total, (finite, total)
    assert longest > 64, longest
    print(f'{finite} of {total} starts have a path; the longest chain has {longest} points')


def test_waypoints_are_in_sight_and_a_walker_that_follows_them_arrives():
    """A point walker taking 0.1 m steps towards its current waypoint: no segment to a waypoint meets a wall, it reaches the goal
    from every finite start within 3000 steps, and walks at most the query's value plus one step."""
    calls = far = 0
    ratios = []
    for case in cases():
        starts, ends = [], []
        for p0, g in zip(case.points, case.g):
            if not np.isfinite(g):
                continue
            p, walked, arrived = p0.copy(), 0., False
            for _ in range(3000):
                w, k = path_rule.waypoint(case.world, p, 16, case.table)
                assert k >= 0
                calls += 1
                far += k >= 2
                w = np.array(w, F)
                starts.append(p.copy()); ends.append(w)
                d = np.linalg.norm(w.astype(np.float64) - p)
                if d <= .1:
                    walked += d
                    p = w
                    if bits(w).tolist() == bits(case.goal).tolist():
                        arrived = True
                        break
                else:
                    p = (p + (w.astype(np.float64) - p)*(.1/d)).astype(F)
                    walked += .1
            assert arrived, (p0, p)
            assert walked <= float(g) + .1, (walked, g)
            ratios.append(walked/float(g))
        assert _crossings(np.array(starts), np.array(ends), case.walls) == 0
    assert far >= .5*calls, (far, calls)
    print(f'{len(ratios)} walks, {calls} waypoint calls, index >= 2 in {far/calls:.3f} of them; walked/query: mean {np.mean(ratios):.4f}, max {np.max(ratios):.4f}')


# ---------------------------------------------------------------------------------------------------------------------
# the kernels' own device functions, instantiated on the host
# ---------------------------------------------------------------------------------------------------------------------
def _host(world, p, lookahead=None, max_points=None):
    from megastep_amd import _lib
    geom, cell, free, D, q = world
    h = _lib.lib()
    geom = np.array(geom, np.int32)
    free = np.ascontiguousarray(free, np.uint8)
    D = np.ascontiguousarray(D, F)
    q, p = np.ascontiguousarray(q, F), np.ascontiguousarray(p, F)
    ptr = lambda a: a.ctypes.data
    if lookahead is not None:
        out = np.zeros(2, F)
        k = h.ms_host_nav_waypoint(ptr(geom), cell, ptr(free), ptr(D), ptr(q), ptr(p), lookahead, ptr(out))
        return out, k
    out = np.zeros((max_points, 2), F)
    count = h.ms_host_nav_path(ptr(geom), cell, ptr(free), ptr(D), ptr(q), ptr(p), max_points, ptr(out))
    return out, count


def _same(world, p, table, lookaheads=(16,), max_points=(8,)):
    for L in lookaheads:
        got, k = _host(world, p, lookahead=L)
        want, wk = path_rule.waypoint(world, p, L, table)
        assert k == wk and bits(got).tolist() == bits(np.array(want, F)).tolist(), (p, L, k, wk)
    for M in max_points:
        got, count = _host(world, p, max_points=M)
        want, wcount = path_rule.path(world, p, M, table)
        assert count == wcount and np.array_equal(bits(got), bits(want)), (p, M, count, wcount)
    return wcount


def test_the_host_instantiations_are_the_rule_bit_for_bit():
    _host_instantiations_are_the_rule(cases())


@pytest.mark.parametrize('cell,r', CELLS)
def test_the_host_instantiations_are_the_rule_at_other_cell_widths(cell, r):
    """The same comparison on the same plans, goals and starts, gridded at cells that are no power of two."""
    found = cases(cell, r)
    assert sum(np.isfinite(case.g).sum() for case in found) >= .8*sum(len(case.g) for case in found)
    assert all(np.isfinite(case.D).sum() > 500 for case in found)
    _host_instantiations_are_the_rule(found)


def _host_instantiations_are_the_rule(found):
    cut = 0
    for case in found:
        for k, p in enumerate(case.points):
            count = _same(case.world, p, case.table, (1, 2, 16, 64) if k % 4 == 0 else (16,), (8, 256) if k % 4 == 0 else (8,))
            cut += count > 8
        # points in walls, outside the grid, not numbers
        lo, hi = case.walls.reshape(-1, 2).min(0), case.walls.reshape(-1, 2).max(0)
        rng = np.random.RandomState(5)
        odd = [case.walls.reshape(-1, 2, 2).mean(1)[k] for k in range(0, len(case.walls), 7)]
        odd += list(lo - .3 + rng.uniform(0, 1, (40, 2))*(hi - lo + .6))
        odd += [lo - 5., hi + 1e6, [np.nan, 2.], [2., np.inf], [-3e38, 3e38]]
        none = 0
        for p in odd:
            none += _same(case.world, np.array(p, F), case.table, (1, 16, 64)) == 0
        assert 5 <= none < len(odd)
    assert cut > 200                                                     # paths cut at max_points = 8 with their full count


def test_a_stale_or_foreign_field_breaks_the_chain_and_nothing_hangs():
    a, b = cases()[0], cases()[3]
    # a field overwritten with a constant: every start has a path of two points, itself and x_0, and no way on
    flat = (a.geom, CELL, a.free, np.full_like(a.D, 3.), a.goal)
    table = path_rule.hops(flat)
    for p in a.points[:20]:
        assert _same(flat, p, table, (1, 16), (8,)) in (-2, 0)
    assert sum(path_rule.path(flat, p, 8, table)[1] == -2 for p in a.points[:20]) >= 16
    # the field of another goal: the chain runs down to THAT goal's cells and stops there, for want of its own
    other = a.points[np.isfinite(a.g)][0]
    foreign = (a.geom, CELL, a.free, nav_rule.field(a.free, a.geom, CELL, other), a.goal)
    table = path_rule.hops(foreign)
    counts = [_same(foreign, p, table, (16, 64), (8,)) for p in a.points[:20]]
    assert min(counts) < -8 and max(counts) <= 0
    # garbage: NaNs, infinities and negative numbers over the field
    rng = np.random.RandomState(3)
    D = b.D.copy()
    D[rng.rand(*D.shape) < .05] = np.nan
    D[rng.rand(*D.shape) < .05] = -np.inf
    D[rng.rand(*D.shape) < .05] = -2.
    junk = (b.geom, CELL, b.free, D, b.goal)
    table = path_rule.hops(junk)
    for p in b.points[:30]:
        _same(junk, p, table, (16, 64), (8, 64))


def test_a_point_on_a_cell_centre_beside_a_wall_is_sent_on_to_the_next_cell():
    """Standing exactly on x_0 next to a wall, nothing further is in sight (every sample's block of four holds a blocked cell):
    the base index 1 keeps the walker from being sent to where it stands."""
    found = 0
    for case in cases()[3:]:                                             # the oblique plans
        ny, nx = case.free.shape
        kind = case.table[0]
        for i in range(1, ny - 1):
            for j in range(1, nx - 1):
                if not (case.free[i, j] and np.isfinite(case.D[i, j]) and kind[i, j] == 1 and not case.free[i - 1:i + 2, j - 1:j + 2].all()):
                    continue
                p = np.array(path_rule.centre(case.geom, CELL, i, j), F)
                points, _, leg0, _ = path_rule.chain(case.world, p, 16, case.table)
                if leg0 != 0 or len(points) < 3:
                    continue
                xs, ys = (np.array([pt[a] for pt in points[1:]], F) for a in (0, 1))
                if path_rule.sights(case.world, p, xs, ys).any():
                    continue
                found += 1
                w, k = path_rule.waypoint(case.world, p, 16, case.table)
                assert k == 1 and w == points[1] and (w[0] != p[0] or w[1] != p[1])
                got, hk = _host(case.world, p, lookahead=16)
                assert hk == 1 and bits(got).tolist() == bits(np.array(w, F)).tolist()
                if found >= 5:
                    return
    assert found > 0


# ---------------------------------------------------------------------------------------------------------------------
# header, loader, refusals
# ---------------------------------------------------------------------------------------------------------------------
PATH_SYMBOLS = {'ms_nav_waypoints', 'ms_nav_paths'}
HOST_SYMBOLS = {'ms_host_nav_waypoint', 'ms_host_nav_path'}


def test_the_header_declares_the_path_calls_and_the_loader_binds_them():
    from megastep_amd import _lib
    assert PATH_SYMBOLS <= set(declared_symbols(('megastep_hip.h',)))
    assert HOST_SYMBOLS <= set(declared_symbols(('megastep_hip_test.h',)))
    assert PATH_SYMBOLS | HOST_SYMBOLS <= set(_lib.SYMBOLS)
    text = open(os.path.join(ROOT, 'include', 'megastep_hip.h')).read()
    assert int(re.search(r'#define MS_ABI_VERSION (\d+)', text).group(1)) == _lib.ABI_VERSION == 17
    handle = _lib.lib()
    assert all(hasattr(handle, s) for s in PATH_SYMBOLS | HOST_SYMBOLS) and handle.ms_abi_version() == 17


@pytest.mark.parametrize('name,fields', [
    ('MsNavWaypoints', ('n_points', 'points', 'goal', 'fields', 'goals', 'n_goals', 'lookahead', 'waypoints', 'hops')),
    ('MsNavPaths', ('n_points', 'points', 'goal', 'fields', 'goals', 'n_goals', 'max_points', 'paths', 'counts'))])
def test_the_path_mirrors_have_the_c_layout(name, fields):
    import subprocess
    import tempfile
    from megastep_amd import _lib
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "megastep_hip.h"\nint main(){printf("%zu", sizeof(' + name + '));' +
           ''.join(f'printf(" %zu", offsetof({name}, {f}));' for f in fields) + '}')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, 't.c'), 'w').write(src)
        subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), os.path.join(d, 't.c'), '-o', os.path.join(d, 't')])
        got = list(map(int, subprocess.check_output([os.path.join(d, 't')]).split()))
    mirror = getattr(_lib, name)
    assert [f for f, _ in mirror._fields_] == list(fields)
    assert got == [ctypes.sizeof(mirror)] + [getattr(mirror, f).offset for f in fields]


def test_bad_path_arguments_are_refused_before_any_launch():
    from megastep_amd import _lib
    h = _lib.lib()
    fake = 64                                       # (never dereferenced: every call below fails its checks first)
    grid = dict(n_envs=2, cell=.125, clearance=.106, geom=fake, starts=fake, max_framed=100, free_cells=fake)
    way = dict(n_points=1, points=fake, goal=None, fields=fake, goals=fake, n_goals=1, lookahead=16, waypoints=fake, hops=None)
    path = dict(n_points=1, points=fake, goal=None, fields=fake, goals=fake, n_goals=1, max_points=8, paths=fake, counts=fake)
    G, W, P = _lib.MsNavGrid, _lib.MsNavWaypoints, _lib.MsNavPaths
    ref = ctypes.byref
    assert h.ms_nav_waypoints(None, ref(W(**way)), None) == -1
    assert h.ms_nav_waypoints(ref(G(**grid)), None, None) == -1
    assert h.ms_nav_paths(None, ref(P(**path)), None) == -1
    assert h.ms_nav_paths(ref(G(**grid)), None, None) == -1
    for bad in (dict(n_envs=0), dict(cell=0.), dict(cell=float('nan')), dict(clearance=0.), dict(cell=.15), dict(geom=None),
                dict(starts=None), dict(free_cells=None), dict(max_framed=-1), dict(geom=68)):
        g = G(**{**grid, **bad})
        assert h.ms_nav_waypoints(ref(g), ref(W(**way)), None) == -1, bad
        assert h.ms_nav_paths(ref(g), ref(P(**path)), None) == -1, bad
    both = (dict(n_points=0), dict(n_points=-1), dict(n_goals=0), dict(n_goals=-3), dict(points=None), dict(fields=None), dict(goals=None),
            dict(n_points=2), dict(points=68), dict(goals=68), dict(fields=66), dict(goal=66))
    for bad in both + (dict(lookahead=0), dict(lookahead=-1), dict(lookahead=65), dict(waypoints=None), dict(waypoints=68), dict(hops=66)):
        assert h.ms_nav_waypoints(ref(G(**grid)), ref(W(**{**way, **bad})), None) == -1, bad
    for bad in both + (dict(max_points=1), dict(max_points=0), dict(max_points=-4), dict(paths=None), dict(counts=None), dict(paths=66),
                       dict(counts=66)):
        assert h.ms_nav_paths(ref(G(**grid)), ref(P(**{**path, **bad})), None) == -1, bad
    # the host instantiations: a look-ahead out of range, fewer than two points
    case = cases()[0]
    assert _host(case.world, case.points[0], lookahead=0)[1] == -2 and _host(case.world, case.points[0], lookahead=65)[1] == -2
    assert _host(case.world, case.points[0], max_points=1)[1] == 0


# ---------------------------------------------------------------------------------------------------------------------
# the follower's rule and the Python calls' refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_the_follower_walks_when_the_waypoint_is_ahead_and_turns_towards_it_otherwise():
    from megastep_amd import modules
    nan = float('nan')
    t = float(np.tan(np.deg2rad(45.)))
    local = torch.tensor([[[0., 2.], [-1., -1.], [1., -1.], [1., 1.], [-1., 1.], [1.01, 1.], [-1.01, 1.], [nan, nan], [0., 0.], [-.5, 0.], [.5, 0.]]])
    assert t == pytest.approx(1.)
    got = modules.PathFollower.choose(local)
    # ahead; behind left; behind right; on the cone's edges (still forward); just outside them; no path; on the spot; abeam
    assert got.dtype == torch.int64 and got.tolist() == [[1, 5, 6, 1, 1, 6, 5, 0, 6, 5, 6]]
    narrow = modules.PathFollower.choose(local, cone=10.)
    assert narrow.tolist() == [[1, 5, 6, 6, 5, 6, 5, 0, 6, 5, 6]]
    # too fast for a waypoint this near: no more acceleration; the limit is speed*|local|, at least CREEP
    ahead = torch.tensor([[[0., 1.], [0., 1.], [0., .1], [0., .1], [1., -1.], [nan, nan]]])
    velocity = torch.tensor([[[0., 1.9], [0., 2.1], [0., .5], [.9, .7], [0., 9.], [0., 9.]]])
    assert modules.PathFollower.choose(ahead, velocity=velocity).tolist() == [[1, 0, 1, 0, 6, 0]]
    assert modules.PathFollower.choose(ahead, velocity=velocity, speed=None).tolist() == [[1, 1, 1, 1, 6, 0]]
    assert modules.PathFollower.choose(ahead, velocity=velocity, speed=1.).tolist() == [[0, 0, 1, 0, 6, 0]]
    # at a dead stop: a sidestep, the other, back, forward, and round again - whatever the waypoint, unless there is none
    blocked = torch.tensor([[0, 1, 2, 3, 4, 5]])
    assert modules.PathFollower.choose(ahead, blocked=blocked).tolist() == [[1, 3, 4, 2, 1, 0]]
    assert modules.PathFollower.choose(local[:, :6], blocked=blocked + 4).tolist() == [[1, 3, 4, 2, 1, 3]]


def test_the_python_calls_refuse_what_they_cannot_do():
    from megastep_amd import cuda
    geom = np.array([[0, 0, 8, 8], [0, 0, 8, 8]], np.int32)
    starts = np.array([0, 64, 128], np.int64)
    grid = cuda.NavGrid(torch.as_tensor(geom), torch.as_tensor(starts), torch.ones(128, dtype=torch.uint8), CELL, RADIUS, geom, starts)
    fields = cuda.DistanceFields(grid, torch.zeros(2, 3, 2), torch.zeros(3*128))
    pts = torch.zeros(2, 3, 2)
    for call in (fields.waypoints, fields.paths):
        with pytest.raises(RuntimeError, match='GPU'):
            call(pts)
        with pytest.raises(RuntimeError, match=r'\(N, P, 2\)'):
            call(torch.zeros(3, 3, 2))
        with pytest.raises(RuntimeError, match=r'\(N, P, 2\)'):
            call(torch.zeros(2, 3, 3))
        with pytest.raises(RuntimeError, match='3-dimensional'):
            call(torch.zeros(2, 3))
        with pytest.raises(RuntimeError, match='dtype'):
            call(pts.double())
        with pytest.raises(RuntimeError, match='one per field'):
            call(torch.zeros(2, 5, 2))
        with pytest.raises(RuntimeError, match='integer'):
            call(pts, goal=torch.zeros(2, 3))
        with pytest.raises(RuntimeError, match='integer'):
            call(pts, goal=torch.zeros(2, 4, dtype=torch.int64))
        with pytest.raises(RuntimeError, match='integer'):
            call(pts, goal=torch.zeros(2, 3, dtype=torch.bool))        # (a mask mistaken for an index)
    for bad in (0, 65, 2.5):
        with pytest.raises(RuntimeError, match='lookahead'):
            fields.waypoints(pts, lookahead=bad)
    for bad in (1, 0, 3.):
        with pytest.raises(RuntimeError, match='max_points'):
            fields.paths(pts, max_points=bad)
