"""Seeded fields (`ms_nav_seed_fields` / `ms_nav_seed_waypoints` / `ms_nav_seed_paths`, `cuda.seeded_fields`,
`SeenMaps.frontier_fields`, `modules.Frontiers`, `FloorCoverage.expert`) on the CPU: the contract of include/megastep_hip.h
(MsNavSeedFields) restated in binary32 numpy (`seed_rule`, which tests/test_gpu_navseed.py holds the kernels to, bit for bit);
the freedom of schedule it rests on; the host instantiations of the kernels' own per-cell functions against the rule; the edge
cases; a walker that follows the waypoints to a seed; and the C-ABI's declarations, layouts and refusals."""
import ctypes
import heapq
import os
import re

import numpy as np
import pytest
import torch

from tests.test_abi import ROOT, declared_symbols
from tests.test_navfield_host import CELL, CELLS, RADIUS, F, INF, _crossings, _two_rooms, _world, bits, nav_rule, plans, spawn_points
from tests.test_navpath_host import NAN, NEIGHBOURS, path_rule
from tests.test_navseen_host import seen_rule


class seed_rule:
    """The contract in numpy: every operation one binary32 operation, in the order the header gives. A `world` is what the
    following reads of one env and one field: (geom, cell, free (ny, nx) bool, D (ny, nx) float32)."""

    @staticmethod
    def seeds(free, marks, where, among=None):
        """(ny, nx) bool: free, among the cells that may be one, bit 0 of the mark equal to `where`."""
        s = free & ((np.asarray(marks, np.uint8) & 1) == int(where))
        return s if among is None else s & ((np.asarray(among, np.uint8) & 1) == 1)

    @staticmethod
    def field(free, cell, seeds, graph=None):
        """The field by a multi-source heap Dijkstra with binary32 additions: (ny, nx) float32."""
        D = np.full(free.size, INF, F)
        first, v, w = graph if graph is not None else nav_rule._neighbours(free, cell)
        heap = [(0., int(a)) for a in np.nonzero(seeds.reshape(-1))[0]]
        D[seeds.reshape(-1)] = F(0)
        done = np.zeros(free.size, bool)
        while heap:
            d, a = heapq.heappop(heap)
            if done[a]:
                continue
            done[a] = True
            da = D[a]
            for k in range(first[a], first[a + 1]):
                nd = da + w[k]                                          # (binary32 + binary32 -> binary32)
                b = v[k]
                if nd < D[b]:
                    D[b] = nd
                    heapq.heappush(heap, (float(nd), b))
        return D.reshape(free.shape)

    @staticmethod
    def field_by_sweeps(free, cell, seeds):
        u, v, w = nav_rule.edges(free, cell)
        D = np.where(seeds.reshape(-1), F(0), INF).astype(F)
        sweeps = 0
        while True:
            new = D.copy()
            np.minimum.at(new, v, D[u] + w)
            sweeps += 1
            if np.array_equal(new, D):
                return D.reshape(free.shape), sweeps
            D = new

    @staticmethod
    def field_by_random_order(free, cell, seeds, seed, chunks=6):
        u, v, w = nav_rule.edges(free, cell)
        rng = np.random.RandomState(seed)
        D = np.where(seeds.reshape(-1), F(0), INF).astype(F)
        while True:
            before = D.copy()
            for part in np.array_split(rng.permutation(len(u)), chunks):
                np.minimum.at(D, v[part], D[u[part]] + w[part])
            if np.array_equal(before, D):
                return D.reshape(free.shape)

    @staticmethod
    def query(world, p):
        geom, cell, free, D = world
        return nav_rule.query(D, geom, cell, free, p)

    @staticmethod
    def hops(world):
        """path_rule's hop table with the one change: the chain ends on the cells at 0, and no goal's cells end it."""
        geom, cell, free, D = world
        kind, step, best = path_rule.hops((geom, cell, free, D, (NAN, NAN)))
        with np.errstate(invalid='ignore'):
            kind[D == 0] = 0
        return kind, step, best

    @staticmethod
    def chain(world, p, limit=None, table=None):
        """(points, ended, leg(p, x_0), cells): the chain's first `limit` points; ended: its last point is a seed's centre. None
        without a path."""
        geom, cell, free, D = world
        kind, step, _ = table if table is not None else seed_rule.hops(world)
        first = path_rule.start((geom, cell, free, D, None), p)
        if first is None:
            return None
        i, j, leg0 = first
        points, cells, ended = [], [], False
        while True:
            points.append(path_rule.centre(geom, cell, i, j)); cells.append((i, j))
            if limit is not None and len(points) >= limit:
                break
            assert len(cells) <= D.size
            if kind[i, j] == 0:
                ended = True
            if kind[i, j] != 1:
                break
            di, dj = NEIGHBOURS[step[i, j]]
            i, j = i + di, j + dj
        return points, ended, leg0, cells

    @staticmethod
    def waypoint(world, p, lookahead=16, table=None):
        geom, cell, free, D = world
        found = seed_rule.chain(world, p, lookahead, table)
        if found is None:
            return (NAN, NAN), -1
        points, _, leg0, _ = found
        n = len(points)
        b = 1 if leg0 <= F(.5)*F(cell) and n >= 2 else 0
        k = b
        if n - 1 > b:
            xs, ys = (np.array([pt[a] for pt in points[b + 1:]], F) for a in (0, 1))
            admissible = np.nonzero(path_rule.sights((geom, cell, free, D, None), p, xs, ys))[0]
            if len(admissible):
                k = b + 1 + int(admissible[-1])
        return points[k], k

    @staticmethod
    def path(world, p, max_points, table=None):
        out = np.full((max_points, 2), NAN, F)
        found = seed_rule.chain(world, p, None, table)
        if found is None:
            return out, 0
        points, ended, _, _ = found
        points = [(F(p[0]), F(p[1]))] + points
        m = min(len(points), max_points)
        out[:m] = np.array(points[:m], F)
        return out, len(points) if ended else -len(points)


# ---------------------------------------------------------------------------------------------------------------------
# the host instantiations
# ---------------------------------------------------------------------------------------------------------------------
_SPARE = np.zeros(8, np.uint8)


def host_field(geom, cell, free, marks, where, among=None, framed=0):
    """ms_host_nav_seed_field: (D (ny, nx), n_seeds, sweeps)."""
    from megastep_amd import _lib
    h = _lib.lib()
    geom = np.array(geom, np.int32)
    free, marks = np.ascontiguousarray(free, np.uint8), np.ascontiguousarray(marks, np.uint8)
    among = None if among is None else np.ascontiguousarray(among, np.uint8)
    D = np.full(free.shape, -7., F)
    n = ctypes.c_int(-7)
    ptr = lambda a: None if a is None else (a.ctypes.data or _SPARE.ctypes.data)
    sweeps = h.ms_host_nav_seed_field(ptr(geom), cell, ptr(free), ptr(marks), int(where), ptr(among), framed, ptr(D), ctypes.addressof(n))
    return D, n.value, sweeps


def host_follow(world, p, lookahead=None, max_points=None):
    from megastep_amd import _lib
    geom, cell, free, D = world
    h = _lib.lib()
    geom = np.array(geom, np.int32)
    free, D, p = np.ascontiguousarray(free, np.uint8), np.ascontiguousarray(D, F), np.ascontiguousarray(p, F)
    ptr = lambda a: a.ctypes.data or _SPARE.ctypes.data
    if lookahead is not None:
        out = np.zeros(2, F)
        k = h.ms_host_nav_seed_waypoint(ptr(geom), cell, ptr(free), ptr(D), ptr(p), lookahead, ptr(out))
        return out, k
    out = np.zeros((max_points, 2), F)
    count = h.ms_host_nav_seed_path(ptr(geom), cell, ptr(free), ptr(D), ptr(p), max_points, ptr(out))
    return out, count


def _same(world, p, table, lookaheads=(16,), max_points=(8,)):
    for L in lookaheads:
        got, k = host_follow(world, p, lookahead=L)
        want, wk = seed_rule.waypoint(world, p, L, table)
        assert k == wk and bits(got).tolist() == bits(np.array(want, F)).tolist(), (p, L, k, wk)
    for M in max_points:
        got, count = host_follow(world, p, max_points=M)
        want, wcount = seed_rule.path(world, p, M, table)
        assert count == wcount and np.array_equal(bits(got), bits(want)), (p, M, count, wcount)
    return wk, wcount


# ---------------------------------------------------------------------------------------------------------------------
# the inputs: three plain and three oblique plans; on each a ring of rays from a spawn point, followed for RANGE metres, and the
# two seed sets it makes - the free cells it has not seen (where = 0, among the free cells) and the ones it has (where = 1)
# ---------------------------------------------------------------------------------------------------------------------
RANGE = 3.


def ring_distances(origin, dirs, walls):
    """How far each ray from `origin` gets before it meets a wall (float64, then rounded; +inf: none)."""
    o, d = np.asarray(origin, np.float64), np.asarray(dirs, np.float64)
    best = np.full(len(d), np.inf)
    for a, b in np.asarray(walls, np.float64).reshape(-1, 2, 2):
        e = b - a
        den = d[:, 0]*e[1] - d[:, 1]*e[0]
        with np.errstate(divide='ignore', invalid='ignore'):
            t = ((a[0] - o[0])*e[1] - (a[1] - o[1])*e[0])/den
            s = ((a[0] - o[0])*d[:, 1] - (a[1] - o[1])*d[:, 0])/den
        hit = (den != 0) & (t > 0) & (s >= 0) & (s <= 1)
        best = np.where(hit & (t < best), t, best)
    return best.astype(F)


def ring_seen(walls, geom, free, origin, n=360, max_range=RANGE, cell=CELL):
    """(ny, nx) uint8: the seen map of a ring of n rays round `origin`, by seen_rule."""
    angle = 2*np.pi*(np.arange(n) + .5)/n
    dirs = np.stack([np.cos(angle), np.sin(angle)], -1).astype(F)
    distances = ring_distances(origin, dirs, walls)
    maps, _, _ = seen_rule.call(geom, cell, free, np.zeros((1,) + free.shape, np.uint8), [0], np.asarray(origin, F)[None], dirs[None],
                                distances[None], max_range=max_range)
    return maps[0]


class _Case:
    """One plan and one seed set."""

    def __init__(self, g, walls, geom, free, graph, marks, where, among, cell=CELL):
        self.g, self.walls, self.geom, self.free, self.marks, self.where, self.among = g, walls, geom, free, marks, where, among
        self.seeds = seed_rule.seeds(free, marks, where, among)
        self.cell = cell
        self.D = seed_rule.field(free, cell, self.seeds, graph)
        self.world = (geom, cell, free, self.D)
        self.table = seed_rule.hops(self.world)
        self.points = spawn_points(g)


_CASES = {}


def cases(cell=CELL, r=RADIUS):
    if (cell, r) not in _CASES:
        rng = np.random.RandomState(41)
        found = _CASES[cell, r] = []
        for g in plans(3) + plans(3, oblique=True):
            walls, geom, free = _world(g, cell, r)
            pts = spawn_points(g)
            origin = (pts[rng.randint(len(pts))] + rng.uniform(-.05, .05, 2)).astype(F)
            seen = ring_seen(walls, geom, free, origin, cell=cell)
            graph = nav_rule._neighbours(free, cell)
            found.append(_Case(g, walls, geom, free, graph, seen, 0, free.astype(np.uint8), cell))
            found.append(_Case(g, walls, geom, free, graph, seen, 1, None, cell))
    return _CASES[cell, r]


def test_most_seed_sets_are_worth_comparing():
    """The condition that keeps the equalities below from being vacuous, met by the numpy rule alone: at least 90 % of the
    (plan, seed set) pairs have a seed and more than 500 finite cells."""
    good = sum(bool(c.seeds.any()) and np.isfinite(c.D).sum() > 500 for c in cases())
    assert good >= .9*len(cases()), (good, len(cases()))
    # both kinds: some of the floor is seen, some is not
    assert all(0 < c.seeds.sum() < c.free.sum() for c in cases())


# ---------------------------------------------------------------------------------------------------------------------
# the rule itself
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('oblique', [False, True])
def test_any_schedule_ends_on_the_same_bits(oblique):
    """Multi-source Dijkstra, synchronous sweeps and a seeded random order of the edges: equal as uint32, infinities included;
    and the field of many seeds is the elementwise minimum of the fields of each - checked on a handful."""
    rng = np.random.RandomState(6)
    for k, g in enumerate(plans(4, oblique)):
        walls, geom, free = _world(g)
        pts = spawn_points(g)
        seen = ring_seen(walls, geom, free, pts[rng.randint(len(pts))])
        seeds = seed_rule.seeds(free, seen, 0, free)
        graph = nav_rule._neighbours(free, CELL)
        want = seed_rule.field(free, CELL, seeds, graph)
        swept, sweeps = seed_rule.field_by_sweeps(free, CELL, seeds)
        shuffled = seed_rule.field_by_random_order(free, CELL, seeds, seed=k)
        assert seeds.sum() > 100 and np.isfinite(want).sum() > 500 and sweeps > 5
        assert np.array_equal(bits(want), bits(swept))
        assert np.array_equal(bits(want), bits(shuffled))
        assert np.isinf(want[~free]).all() and np.array_equal(want == 0, seeds)
        # a handful of seeds: the minimum of their own fields
        few = np.zeros(free.size, bool)
        few[rng.choice(np.nonzero(free.reshape(-1))[0], 5, replace=False)] = True
        few = few.reshape(free.shape)
        each = []
        for a in np.nonzero(few.reshape(-1))[0]:
            one = np.zeros(free.size, bool)
            one[a] = True
            each.append(seed_rule.field(free, CELL, one.reshape(free.shape), graph))
        together = seed_rule.field(free, CELL, few, graph)
        assert np.array_equal(bits(together), bits(np.minimum.reduce(each)))
        assert np.isfinite(together).sum() > 500


# ---------------------------------------------------------------------------------------------------------------------
# the kernels' own per-cell functions, instantiated on the host
# ---------------------------------------------------------------------------------------------------------------------
def test_the_host_field_is_the_rule_bit_for_bit():
    _host_field_is_the_rule(cases())


def _worth_comparing(found):
    """At least 90 % of the seed sets have a seed and more than 500 finite cells, and every plan is partly seen."""
    good = sum(bool(c.seeds.any()) and np.isfinite(c.D).sum() > 500 for c in found)
    assert good >= .9*len(found), (good, len(found))
    assert all(0 < c.seeds.sum() < c.free.sum() for c in found)


@pytest.mark.parametrize('cell,r', CELLS)
def test_the_host_field_is_the_rule_at_other_cell_widths(cell, r):
    _worth_comparing(cases(cell, r))
    _host_field_is_the_rule(cases(cell, r))


def _host_field_is_the_rule(found):
    for case in found:
        for framed in (0, 1):
            D, n, sweeps = host_field(case.geom, case.cell, case.free, case.marks, case.where, case.among, framed)
            assert n == case.seeds.sum() and sweeps >= 2
            assert np.array_equal(bits(D), bits(case.D)), (framed, int((bits(D) != bits(case.D)).sum()))
        # marks and among are read by their bit 0 alone
        noisy = case.marks | ((np.arange(case.marks.size) % 128).astype(np.uint8).reshape(case.marks.shape) << 1)
        among = None if case.among is None else case.among | 6
        assert np.array_equal(bits(host_field(case.geom, case.cell, case.free, noisy, case.where, among)[0]), bits(case.D))


def test_the_host_followers_are_the_rule_bit_for_bit():
    """From every spawn point of every case; a subset with other look-aheads and path lengths; then points in walls, outside
    the grid and not numbers."""
    _host_followers_are_the_rule(cases(), 1)


@pytest.mark.parametrize('cell,r', CELLS)
def test_the_host_followers_are_the_rule_at_other_cell_widths(cell, r):
    """From every eighth spawn point of the same plans and seed sets, gridded at cells that are no power of two."""
    _worth_comparing(cases(cell, r))
    _host_followers_are_the_rule(cases(cell, r), 8)


def _host_followers_are_the_rule(found, stride):
    on_seed = cut = finite = total = 0
    for case in found:
        for k, p in enumerate(case.points[::stride]):
            many = k % 16 == 0
            hops, count = _same(case.world, p, case.table, (1, 2, 16, 64) if many else (16,), (8, 256) if many else (8,))
            total += 1
            finite += hops >= 0
            on_seed += hops == 0
            cut += count > 8
            assert (hops < 0) == (count == 0) == bool(np.isinf(seed_rule.query(case.world, p)))
            assert count >= 0                                            # (a fixed point never breaks a chain)
        lo, hi = case.walls.reshape(-1, 2).min(0), case.walls.reshape(-1, 2).max(0)
        rng = np.random.RandomState(5)
        odd = [case.walls.reshape(-1, 2, 2).mean(1)[k] for k in range(0, len(case.walls), 7)]
        odd += list(lo - .3 + rng.uniform(0, 1, (40, 2))*(hi - lo + .6))
        odd += [lo - 5., hi + 1e6, [np.nan, 2.], [2., np.inf], [-3e38, 3e38]]
        none = sum(_same(case.world, np.array(p, F), case.table, (1, 16, 64))[1] == 0 for p in odd)
        assert 5 <= none < len(odd)
    assert finite >= .8*total and on_seed > 100/stride and cut > 100/stride, (finite, total, on_seed, cut)


def test_a_stale_or_garbage_field_breaks_the_chain_and_nothing_hangs():
    a = cases()[0]
    flat = (a.geom, CELL, a.free, np.full_like(a.D, 3.))
    table = seed_rule.hops(flat)
    counts = [_same(flat, p, table, (1, 16), (8,))[1] for p in a.points[:20]]
    assert set(counts) <= {-2, 0} and counts.count(-2) >= 16
    rng = np.random.RandomState(3)
    D = a.D.copy()
    D[rng.rand(*D.shape) < .05] = np.nan
    D[rng.rand(*D.shape) < .05] = -np.inf
    D[rng.rand(*D.shape) < .05] = -2.
    D[rng.rand(*D.shape) < .02] = 0.                                    # (zeros on blocked cells too: no anchor, no neighbour)
    junk = (a.geom, CELL, a.free, D)
    table = seed_rule.hops(junk)
    for p in a.points[:40]:
        _same(junk, p, table, (16, 64), (8, 64))


# ---------------------------------------------------------------------------------------------------------------------
# edge cases
# ---------------------------------------------------------------------------------------------------------------------
def _nothing(case, marks, where, among):
    """A field without a seed: +inf throughout, and nothing to follow."""
    assert not seed_rule.seeds(case.free, marks, where, among).any()
    for framed in (0, 1):
        D, n, sweeps = host_field(case.geom, CELL, case.free, marks, where, among, framed)
        assert n == 0 and sweeps == 1 and np.isinf(D).all() and (D > 0).all()
    world = (case.geom, CELL, case.free, D)
    table = seed_rule.hops(world)
    for p in case.points[:10]:
        assert _same(world, p, table, (1, 16), (8,)) == (-1, 0)
        way, k = host_follow(world, p, lookahead=16)
        assert np.isnan(way).all() and k == -1 and np.isnan(host_follow(world, p, max_points=4)[0]).all()


def test_no_seed_seeds_on_blocked_cells_only_and_an_empty_among():
    case = cases()[0]
    ones, zeros = np.ones(case.free.shape, np.uint8), np.zeros(case.free.shape, np.uint8)
    _nothing(case, ones, 0, None)
    _nothing(case, zeros, 1, None)
    _nothing(case, (~case.free).astype(np.uint8), 1, None)              # marked on blocked cells only
    _nothing(case, case.free.astype(np.uint8), 0, None)                 # unmarked on blocked cells only
    _nothing(case, case.marks, case.where, zeros)                       # among: nobody
    _nothing(case, case.marks, case.where, zeros + 2)                   # (bit 0 is what counts)


def test_an_env_without_cells():
    none = np.zeros((0, 0), np.uint8)
    for geom in ((0, 0, 0, 0), (3, 4, 0, 7)):
        D, n, sweeps = host_field(geom, CELL, none, none, 1)
        assert n == 0 and sweeps == 0
        world = (geom, CELL, none.astype(bool), np.zeros((0, 0), F))
        way, k = host_follow(world, (1., 1.), lookahead=16)
        assert np.isnan(way).all() and k == -1
        pts, count = host_follow(world, (1., 1.), max_points=4)
        assert np.isnan(pts).all() and count == 0


def test_a_start_whose_anchor_is_a_seed_is_sent_to_it():
    found = 0
    for case in cases():
        for p in case.points:
            first = path_rule.start((case.geom, CELL, case.free, case.D, None), p)
            if first is None or not case.seeds[first[0], first[1]]:
                continue
            found += 1
            centre = np.array(path_rule.centre(case.geom, CELL, first[0], first[1]), F)
            way, k = host_follow(case.world, p, lookahead=16)
            assert k == 0 and bits(way).tolist() == bits(centre).tolist()
            pts, count = host_follow(case.world, p, max_points=4)
            assert count == 2 and bits(pts[0]).tolist() == bits(p).tolist() and bits(pts[1]).tolist() == bits(centre).tolist()
            assert np.isnan(pts[2:]).all()
            if found % 50 == 0:
                break
    assert found > 20


def test_a_sealed_room_has_no_way_to_the_seeds_next_door():
    walls, a, b, (j0, j1) = _two_rooms()
    geom = nav_rule.geometry(walls, CELL)
    marks = np.zeros((geom[3], geom[2]), np.uint8)
    corner = path_rule.corner(b, geom, CELL)
    marks[corner[0] - 2:corner[0] + 3, corner[1] - 2:corner[1] + 3] = 1  # a patch of seeds round b, in the right room
    for shut in (False, True):
        w = np.concatenate([walls, np.array([[j0, j1]], F)]) if shut else walls
        free = nav_rule.free(w, geom, CELL, RADIUS)
        seeds = seed_rule.seeds(free, marks, 1)
        assert seeds.sum() == 25
        want = seed_rule.field(free, CELL, seeds)
        D, n, _ = host_field(geom, CELL, free, marks, 1, framed=int(shut))
        assert n == 25 and np.array_equal(bits(D), bits(want)) and np.isfinite(D).sum() > 500
        world = (geom, CELL, free, D)
        hops, count = _same(world, a, seed_rule.hops(world), (16,), (256,))
        if shut:
            assert (hops, count) == (-1, 0) and np.isinf(seed_rule.query(world, a))
            assert np.isnan(host_follow(world, a, lookahead=16)[0]).all()
        else:
            path, count = host_follow(world, a, max_points=256)
            assert hops >= 2 and 2 < count <= 256
            assert _crossings(path[:count - 1], path[1:count], walls) == 0
            assert np.linalg.norm(path[:count] - (j0 + j1)/2, axis=1).min() <= .5      # through the door
            assert seeds[path_rule.corner(path[count - 1] + F(CELL/2), geom, CELL)]     # (it ends on a seed's centre)


# ---------------------------------------------------------------------------------------------------------------------
# a walker
# ---------------------------------------------------------------------------------------------------------------------
def test_a_walker_that_follows_the_waypoints_reaches_a_seed():
    """A point walker taking 0.1 m steps towards its current waypoint: from every start with a finite distance it ends on the
    centre of a cell at 0, no segment to a waypoint meets a wall, and it walks no further than the field said at its start plus
    one cell diagonal."""
    rng = np.random.RandomState(9)
    walks = 0
    diagonal = float(F(CELL))*2**.5
    for case in cases():
        starts, ends = [], []
        for p0 in case.points[rng.choice(len(case.points), 24, replace=False)]:
            g = seed_rule.query(case.world, p0)
            if not np.isfinite(g):
                continue
            p, walked, arrived = p0.copy(), 0., False
            for _ in range(3000):
                w, k = seed_rule.waypoint(case.world, p, 16, case.table)
                assert k >= 0
                w = np.array(w, F)
                starts.append(p.copy()); ends.append(w)
                d = np.linalg.norm(w.astype(np.float64) - p)
                if d <= .1:
                    walked += d
                    p = w
                    i, j = path_rule.corner(p + F(CELL/2), case.geom, CELL)      # (p is a centre: the cell it is the centre of)
                    if case.D[i, j] == 0 and bits(np.array(path_rule.centre(case.geom, CELL, i, j), F)).tolist() == bits(p).tolist():
                        arrived = True
                        break
                else:
                    p = (p + (w.astype(np.float64) - p)*(.1/d)).astype(F)
                    walked += .1
            assert arrived, (p0, p)
            assert walked <= float(g) + diagonal, (walked, g)
            walks += 1
        assert _crossings(np.array(starts), np.array(ends), case.walls) == 0
    assert walks > 200


# ---------------------------------------------------------------------------------------------------------------------
# header, loader, refusals
# ---------------------------------------------------------------------------------------------------------------------
SEED_SYMBOLS = {'ms_nav_seed_fields', 'ms_nav_seed_waypoints', 'ms_nav_seed_paths'}
HOST_SYMBOLS = {'ms_host_nav_seed_field', 'ms_host_nav_seed_waypoint', 'ms_host_nav_seed_path', 'ms_host_nav_field_capacity'}


def test_the_relaxations_capacities_are_the_librarys():
    """cuda.FIELD_CAPACITY is what nav_relax_kernel's three instantiations hold, in framed cells: a float and a byte a cell in
    40, 80 and 160 KiB less the flags, a multiple of four."""
    from megastep_amd import _lib, cuda, nav
    caps = (ctypes.c_int*3)()
    assert _lib.lib().ms_host_nav_field_capacity(caps) == 0 and tuple(caps) == nav.FIELD_CAPACITY == (8176, 16368, 32752)
    assert tuple(caps) == tuple((kib*1024 - 64)//5//4*4 for kib in (40, 80, 160))
    assert _lib.lib().ms_host_nav_field_capacity(None) == -1
    assert cuda.FIELD_CAPACITY is nav.FIELD_CAPACITY


def test_the_header_declares_the_seeded_calls_and_the_loader_binds_them():
    from megastep_amd import _lib
    assert SEED_SYMBOLS <= set(declared_symbols(('megastep_hip.h',)))
    assert HOST_SYMBOLS <= set(declared_symbols(('megastep_hip_test.h',)))
    assert SEED_SYMBOLS | HOST_SYMBOLS <= set(_lib.SYMBOLS)
    text = open(os.path.join(ROOT, 'include', 'megastep_hip.h')).read()
    assert int(re.search(r'#define MS_ABI_VERSION (\d+)', text).group(1)) == _lib.ABI_VERSION == 17
    handle = _lib.lib()
    assert all(hasattr(handle, s) for s in SEED_SYMBOLS | HOST_SYMBOLS) and handle.ms_abi_version() == 17


@pytest.mark.parametrize('name,fields', [
    ('MsNavSeedFields', ('n_fields', 'marks', 'where', 'among', 'mask', 'fields', 'passes', 'n_seeds')),
    ('MsNavSeedWaypoints', ('n_points', 'points', 'goal', 'fields', 'n_goals', 'lookahead', 'waypoints', 'hops')),
    ('MsNavSeedPaths', ('n_points', 'points', 'goal', 'fields', 'n_goals', 'max_points', 'paths', 'counts'))])
def test_the_seeded_mirrors_have_the_c_layout(name, fields):
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


def test_bad_seeded_arguments_are_refused_before_any_launch():
    from megastep_amd import _lib
    h = _lib.lib()
    fake = 64                                       # (never dereferenced: every call below fails its checks first)
    grid = dict(n_envs=2, cell=.125, clearance=.106, geom=fake, starts=fake, max_framed=100, free_cells=fake)
    seed = dict(n_fields=1, marks=fake, where=0, among=None, mask=None, fields=fake, passes=None, n_seeds=None)
    way = dict(n_points=1, points=fake, goal=None, fields=fake, n_goals=1, lookahead=16, waypoints=fake, hops=None)
    path = dict(n_points=1, points=fake, goal=None, fields=fake, n_goals=1, max_points=8, paths=fake, counts=fake)
    G, S, W, P = _lib.MsNavGrid, _lib.MsNavSeedFields, _lib.MsNavSeedWaypoints, _lib.MsNavSeedPaths
    ref = ctypes.byref
    calls = ((h.ms_nav_seed_fields, S, seed), (h.ms_nav_seed_waypoints, W, way), (h.ms_nav_seed_paths, P, path))
    for call, kind, good in calls:
        assert call(None, ref(kind(**good)), None) == -1
        assert call(ref(G(**grid)), None, None) == -1
        for bad in (dict(n_envs=0), dict(cell=0.), dict(cell=float('nan')), dict(clearance=0.), dict(cell=.15), dict(geom=None),
                    dict(starts=None), dict(free_cells=None), dict(max_framed=-1), dict(geom=68)):
            assert call(ref(G(**{**grid, **bad})), ref(kind(**good)), None) == -1, bad
    for bad in (dict(n_fields=0), dict(n_fields=-2), dict(marks=None), dict(fields=None), dict(where=2), dict(where=-1), dict(where=256),
                dict(fields=66), dict(passes=66), dict(n_seeds=66)):
        assert h.ms_nav_seed_fields(ref(G(**grid)), ref(S(**{**seed, **bad})), None) == -1, bad
    both = (dict(n_points=0), dict(n_points=-1), dict(n_goals=0), dict(n_goals=-3), dict(points=None), dict(fields=None), dict(n_points=2),
            dict(points=68), dict(fields=66), dict(goal=66))
    for bad in both + (dict(lookahead=0), dict(lookahead=-1), dict(lookahead=65), dict(waypoints=None), dict(waypoints=68), dict(hops=66)):
        assert h.ms_nav_seed_waypoints(ref(G(**grid)), ref(W(**{**way, **bad})), None) == -1, bad
    for bad in both + (dict(max_points=1), dict(max_points=0), dict(max_points=-4), dict(paths=None), dict(counts=None), dict(paths=66),
                       dict(counts=66)):
        assert h.ms_nav_seed_paths(ref(G(**grid)), ref(P(**{**path, **bad})), None) == -1, bad
    # the host instantiations
    case = cases()[0]
    geom, free, marks = np.array(case.geom, np.int32), np.ascontiguousarray(case.free, np.uint8), np.ascontiguousarray(case.marks, np.uint8)
    D = np.zeros(case.free.shape, F)
    ptr = lambda a: a.ctypes.data
    args = lambda **kw: [kw.get('geom', ptr(geom)), kw.get('cell', CELL), kw.get('free', ptr(free)), kw.get('marks', ptr(marks)),
                         kw.get('where', 1), None, 0, kw.get('D', ptr(D)), None]
    assert h.ms_host_nav_seed_field(*args()) > 0
    for bad in (dict(geom=None), dict(cell=0.), dict(cell=float('inf')), dict(where=2), dict(where=-1), dict(free=None), dict(marks=None), dict(D=None)):
        assert h.ms_host_nav_seed_field(*args(**bad)) == -1, bad
    assert host_follow(case.world, case.points[0], lookahead=0)[1] == -2 and host_follow(case.world, case.points[0], lookahead=65)[1] == -2
    assert host_follow(case.world, case.points[0], max_points=1)[1] == 0


def test_the_python_calls_refuse_what_they_cannot_do():
    from megastep_amd import cuda
    geom = np.array([[0, 0, 8, 8], [0, 0, 8, 8]], np.int32)
    starts = np.array([0, 64, 128], np.int64)
    grid = cuda.NavGrid(torch.as_tensor(geom), torch.as_tensor(starts), torch.ones(128, dtype=torch.uint8), CELL, RADIUS, geom, starts)
    marks = torch.zeros(3*128, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match='GPU'):
        cuda.seeded_fields(grid, marks, 3)
    with pytest.raises(RuntimeError, match='GPU'):
        cuda.seeded_fields(grid, marks.bool(), 3, where=False, among=torch.ones(128, dtype=torch.bool))
    with pytest.raises(RuntimeError, match='GPU'):
        cuda.seen_maps(grid, 3).frontier_fields()
    for bad in (0, -1, 2.5):
        with pytest.raises(RuntimeError, match='n_fields'):
            cuda.seeded_fields(grid, marks, bad)
    for n_fields in (2, 4):                                             # a length that is not n_fields*n_cells
        with pytest.raises(RuntimeError, match='entries'):
            cuda.seeded_fields(grid, marks, n_fields)
    for bad in (marks.float(), marks.int(), marks.reshape(3, 128), marks[::2], list(range(4))):
        with pytest.raises(RuntimeError, match='marks'):
            cuda.seeded_fields(grid, bad, 3)
    for bad in (torch.ones(64, dtype=torch.uint8), torch.ones(128), torch.ones(2, 64, dtype=torch.uint8)):
        with pytest.raises(RuntimeError, match='among'):
            cuda.seeded_fields(grid, marks, 3, among=bad)
    fields = cuda.SeededFields(grid, marks, 3, True, None, torch.zeros(3*128), torch.zeros(2, 3, dtype=torch.int32))
    assert fields.n_goals == fields.n_fields == 3 and fields.image(1, 2).shape == (8, 8)
    for bad in (torch.ones(2, 3), torch.ones(3, 2, dtype=torch.bool), [[True]*3]*2):
        with pytest.raises(RuntimeError, match='mask'):
            fields.update(bad)
    with pytest.raises(RuntimeError, match='GPU'):
        fields.update()
    with pytest.raises(RuntimeError, match='`out`'):
        cuda.seeded_fields(grid, marks, 3, out=cuda.SeededFields(grid, marks.clone(), 3, True, None, fields.values, fields.n_seeds))
    with pytest.raises(RuntimeError, match='`out`'):
        cuda.seeded_fields(grid, marks, 3, where=False, out=fields)
    pts = torch.zeros(2, 3, 2)
    for call in (fields.at, fields.waypoints, fields.paths):
        with pytest.raises(RuntimeError, match='GPU'):
            call(pts)
        with pytest.raises(RuntimeError, match=r'\(N, P, 2\)'):
            call(torch.zeros(3, 3, 2))
        with pytest.raises(RuntimeError, match='3-dimensional'):
            call(torch.zeros(2, 3))
        with pytest.raises(RuntimeError, match='dtype'):
            call(pts.double())
        with pytest.raises(RuntimeError, match='one per field'):
            call(torch.zeros(2, 5, 2))
        with pytest.raises(RuntimeError, match='integer'):
            call(pts, goal=torch.zeros(2, 3))
    for bad in (0, 65, 2.5):
        with pytest.raises(RuntimeError, match='lookahead'):
            fields.waypoints(pts, lookahead=bad)
    for bad in (1, 0, 3.):
        with pytest.raises(RuntimeError, match='max_points'):
            fields.paths(pts, max_points=bad)
