"""Shortest-path distance fields (`ms_nav_free` / `ms_nav_fields` / `ms_nav_query`, `cuda.nav_grid`, `cuda.distance_fields`,
`modules.Goals`, `demo.PointGoal`) on the CPU: the contract of include/megastep_hip.h (MsNavGrid) restated in binary32 numpy
(`nav_rule`, which tests/test_gpu_navfield.py holds the kernels to, bit for bit), the freedom of schedule it rests on, the
promise that no path of the graph passes through a wall, known answers, the C-ABI's declarations, layouts and refusals, and
the envs' bookkeeping against a hand-filled stand-in for the fields."""
import ctypes
import heapq
import os
import re

import numpy as np
import pytest
import torch

from tests.test_abi import ROOT, declared_symbols
from tests.test_overhead_host import line_d2

F = np.float32
INF = F(np.inf)
DIAGONAL = F(1.41421356)
CELL, RADIUS = .125, .15/2**.5          # the defaults: cuda.nav_grid's cell and core.AGENT_RADIUS
# (cell, clearance) pairs whose cell is no power of two - at .125 a centre ((origin + k) + .5)*c, a quotient x/c, a diagonal
# c*1.41421356f, a sample count len/(.5f*c) and an area cells*(c*c) are all exact, so a slip in any of them goes unseen there;
# each has cell <= 1.4*clearance, the last with a clearance that is not the default either.  The nav tests that hold the library
# to a numpy rule run at these too (tests/test_gpu_navcells.py and the `_at_other_cell_widths` tests of the host modules).
CELLS = [(.1, RADIUS), (.14, RADIUS), (.2, .15)]


class nav_rule:
    """The contract in numpy: every operation one binary32 operation, in the order the header gives."""

    @staticmethod
    def geometry(walls, cell):
        """(jx0, iy0, nx, ny) of the grid cuda.nav_grid lays over `walls` (L, 2, 2): their bounding box and a cell of margin."""
        pts = np.asarray(walls, F).reshape(-1, 2).astype(np.float64)
        if not len(pts):
            return 0, 0, 0, 0
        c = float(F(cell))
        first = np.floor(pts.min(0)/c).astype(int) - 1
        last = np.floor(pts.max(0)/c).astype(int) + 1
        return int(first[0]), int(first[1]), int(last[0] - first[0] + 1), int(last[1] - first[1] + 1)

    @staticmethod
    def centres(geom, cell):
        jx0, iy0, nx, ny = geom
        x = ((jx0 + np.arange(nx)).astype(F) + F(.5))*F(cell)
        y = ((iy0 + np.arange(ny)).astype(F) + F(.5))*F(cell)
        return x, y

    @staticmethod
    def free(walls, geom, cell, clearance):
        """(ny, nx) bool: the cells no wall covers at half width `clearance` (MsOverhead's d2 <= r*r; a NaN never covers)."""
        x, y = nav_rule.centres(geom, cell)
        x, y = np.broadcast_arrays(x[None, :], y[:, None])
        h2 = F(clearance)*F(clearance)
        blocked = np.zeros(x.shape, bool)
        for line in np.asarray(walls, F).reshape(-1, 4):
            d2, _ = line_d2(x, y, line)
            with np.errstate(invalid='ignore'):
                blocked |= d2 <= h2
        return ~blocked

    @staticmethod
    def edges(free, cell):
        """(u, v, w): every directed edge of the graph, cells as flat row-major indices."""
        ny, nx = free.shape
        pad = np.zeros((ny + 2, nx + 2), bool)
        pad[1:-1, 1:-1] = free
        idx = np.arange(ny*nx).reshape(ny, nx)
        us, vs, ws = [], [], []
        for di in (-1, 0, 1):
            for dj in (-1, 0, 1):
                if di == 0 and dj == 0:
                    continue
                ok = free & pad[1 + di:ny + 1 + di, 1 + dj:nx + 1 + dj]
                if di and dj:                                           # no corner is cut
                    ok &= pad[1 + di:ny + 1 + di, 1:nx + 1] & pad[1:ny + 1, 1 + dj:nx + 1 + dj]
                i, j = np.nonzero(ok)
                us.append(idx[i, j]); vs.append(idx[i + di, j + dj])
                ws.append(np.full(len(i), F(cell)*DIAGONAL if di and dj else F(cell), F))
        return np.concatenate(us), np.concatenate(vs), np.concatenate(ws)

    @staticmethod
    def anchors(p, geom, cell, free):
        """[(i, j, leg)] of point p."""
        jx0, iy0, nx, ny = geom
        c = F(cell)
        with np.errstate(all='ignore'):
            fx, fy = np.floor(F(p[0])/c - F(.5)), np.floor(F(p[1])/c - F(.5))
        if not (abs(fx) < 2.**30 and abs(fy) < 2.**30):
            return []
        j0, i0 = int(fx) - jx0, int(fy) - iy0
        out = []
        for i in (i0, i0 + 1):
            for j in (j0, j0 + 1):
                if 0 <= i < ny and 0 <= j < nx and free[i, j]:
                    dx = F(p[0]) - (F(jx0 + j) + F(.5))*c
                    dy = F(p[1]) - (F(iy0 + i) + F(.5))*c
                    out.append((i, j, np.sqrt(dx*dx + dy*dy)))
        return out

    @staticmethod
    def _neighbours(free, cell):
        """Per cell the list of (neighbour, weight) as python numbers, for the heap."""
        u, v, w = nav_rule.edges(free, cell)
        order = np.argsort(u, kind='stable')
        u, v, w = u[order], v[order], w[order]
        first = np.searchsorted(u, np.arange(free.size + 1))
        return first, v, w

    @staticmethod
    def field(free, geom, cell, p, graph=None):
        """The field of goal p by a heap Dijkstra with binary32 additions: (ny, nx) float32."""
        D = np.full(free.size, INF, F)
        first, v, w = graph if graph is not None else nav_rule._neighbours(free, cell)
        heap = []
        for i, j, leg in nav_rule.anchors(p, geom, cell, free):
            D[i*free.shape[1] + j] = leg
            heap.append((float(leg), i*free.shape[1] + j))
        heapq.heapify(heap)
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
    def field_by_sweeps(free, geom, cell, p):
        """The same field by synchronous sweeps over all edges at once; returns (field, sweeps)."""
        u, v, w = nav_rule.edges(free, cell)
        D = np.full(free.size, INF, F)
        for i, j, leg in nav_rule.anchors(p, geom, cell, free):
            D[i*free.shape[1] + j] = leg
        sweeps = 0
        while True:
            new = D.copy()
            np.minimum.at(new, v, D[u] + w)
            sweeps += 1
            if np.array_equal(new, D):
                return D.reshape(free.shape), sweeps
            D = new

    @staticmethod
    def field_by_random_order(free, geom, cell, p, seed, chunks=6):
        """The same field by relaxing the edges in a seeded random order, a fresh order every round, each round in a few chunks
        (an edge of a chunk sees what the chunks before it left)."""
        u, v, w = nav_rule.edges(free, cell)
        rng = np.random.RandomState(seed)
        D = np.full(free.size, INF, F)
        for i, j, leg in nav_rule.anchors(p, geom, cell, free):
            D[i*free.shape[1] + j] = leg
        while True:
            before = D.copy()
            for part in np.array_split(rng.permutation(len(u)), chunks):
                np.minimum.at(D, v[part], D[u[part]] + w[part])
            if np.array_equal(before, D):
                return D.reshape(free.shape)

    @staticmethod
    def query(D, geom, cell, free, p):
        best = INF
        for i, j, leg in nav_rule.anchors(p, geom, cell, free):
            best = min(best, D[i, j] + leg)
        return F(best)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def plans(n, oblique=False, large=False, seed=7):
    from megastep_amd import cubicasa
    return cubicasa.sample(n, seed=seed, n_unique=max(16, n), oblique=oblique, large=large)


def spawn_points(g):
    """The centres of the plan's room cells: RandomSpawns' table is drawn from these."""
    from megastep_amd import geometry
    free = np.stack((g['masks'] > 0).nonzero(), -1)
    return geometry.centers(free, g['masks'].shape, g['res']).astype(F)


def _world(g, cell=CELL, r=RADIUS):
    walls = np.asarray(g['walls'], F)
    geom = nav_rule.geometry(walls, cell)
    return walls, geom, nav_rule.free(walls, geom, cell, r)


# ---------------------------------------------------------------------------------------------------------------------
# the rule itself
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('oblique', [False, True])
def test_any_schedule_ends_on_the_same_bits(oblique):
    """Dijkstra, synchronous sweeps and a seeded random order of the edges: equal as uint32, infinities included."""
    rng = np.random.RandomState(3)
    for k, g in enumerate(plans(4, oblique)):
        walls, geom, free = _world(g)
        pts = spawn_points(g)
        p = pts[rng.randint(len(pts))] + rng.uniform(-.05, .05, 2).astype(F)
        want = nav_rule.field(free, geom, CELL, p)
        swept, sweeps = nav_rule.field_by_sweeps(free, geom, CELL, p)
        shuffled = nav_rule.field_by_random_order(free, geom, CELL, p, seed=k)
        assert np.isfinite(want).sum() > 500 and sweeps > 20
        assert np.array_equal(bits(want), bits(swept))
        assert np.array_equal(bits(want), bits(shuffled))
        assert np.isinf(want[~free]).all()


def _crossings(a, b, walls):
    """How many (segment, wall) pairs properly meet, in float64: segments a[k] -> b[k] against every wall."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    total = 0
    for w in np.asarray(walls, np.float64).reshape(-1, 2, 2):
        p, q = w
        d1 = (q[0] - p[0])*(a[:, 1] - p[1]) - (q[1] - p[1])*(a[:, 0] - p[0])
        d2 = (q[0] - p[0])*(b[:, 1] - p[1]) - (q[1] - p[1])*(b[:, 0] - p[0])
        r = b - a
        d3 = r[:, 0]*(p[1] - a[:, 1]) - r[:, 1]*(p[0] - a[:, 0])
        d4 = r[:, 0]*(q[1] - a[:, 1]) - r[:, 1]*(q[0] - a[:, 0])
        total += int(((d1*d2 <= 0) & (d3*d4 <= 0) & ((d1 != d2) | (d3 != d4))).sum())
    return total


def _distance_to_walls(pts, walls):
    pts = np.asarray(pts, np.float64)
    best = np.full(len(pts), np.inf)
    for w in np.asarray(walls, np.float64).reshape(-1, 2, 2):
        v = w[1] - w[0]
        vv = v @ v
        t = np.clip(((pts - w[0]) @ v)/vv, 0, 1) if vv > 0 else np.zeros(len(pts))
        best = np.minimum(best, np.linalg.norm(pts - (w[0] + t[:, None]*v), axis=1))
    return best


def _no_edge_or_leg_crosses(walls, geom, free, cell, r, rng, n_points=1000):
    x, y = nav_rule.centres(geom, cell)
    u, v, _ = nav_rule.edges(free, cell)
    nx = free.shape[1]
    a = np.stack([x[u % nx], y[u // nx]], 1)
    b = np.stack([x[v % nx], y[v // nx]], 1)
    assert len(u) > 1000
    assert _crossings(a, b, walls) == 0
    lo, hi = walls.reshape(-1, 2).min(0), walls.reshape(-1, 2).max(0)
    pts = np.zeros((0, 2), F)
    while len(pts) < n_points:
        cand = (lo + rng.uniform(0, 1, (4*n_points, 2))*(hi - lo)).astype(F)
        pts = np.concatenate([pts, cand[_distance_to_walls(cand, walls) > r]])[:n_points]
    starts, ends = [], []
    for p in pts:
        for i, j, leg in nav_rule.anchors(p, geom, cell, free):
            starts.append(p); ends.append((x[j], y[i]))
    assert len(starts) > n_points
    assert _crossings(np.array(starts), np.array(ends), walls) == 0


@pytest.mark.parametrize('oblique', [False, True])
def test_no_edge_and_no_leg_passes_through_a_wall(oblique):
    rng = np.random.RandomState(11)
    for g in plans(2, oblique):
        walls, geom, free = _world(g)
        _no_edge_or_leg_crosses(walls, geom, free, CELL, RADIUS, rng)


def _two_rooms():
    """Two rooms side by side, parted by a zero-thickness wall at 30 degrees to the vertical whose only opening is a door
    0.5 m wide; returns (walls, a point in the left room, a point in the right room, the door's two jambs)."""
    box = [[[1, 1], [9, 1]], [[9, 1], [9, 6]], [[9, 6], [1, 6]], [[1, 6], [1, 1]]]
    foot, d = np.array([4., 1.]), np.array([np.sin(np.pi/6), np.cos(np.pi/6)])
    length = 5/d[1]
    s0, s1 = .55*length, .55*length + .5
    walls = np.array(box + [[foot, foot + s0*d], [foot + s1*d, foot + length*d]], F)
    return walls, np.array([2., 2.], F), np.array([8., 2.], F), (foot + s0*d, foot + s1*d)


def test_a_thin_oblique_wall_is_walked_round_through_its_door():
    walls, a, b, (j0, j1) = _two_rooms()
    geom = nav_rule.geometry(walls, CELL)
    free = nav_rule.free(walls, geom, CELL, RADIUS)
    _no_edge_or_leg_crosses(walls, geom, free, CELL, RADIUS, np.random.RandomState(5))
    D = nav_rule.field(free, geom, CELL, b)
    g = float(nav_rule.query(D, geom, CELL, free, a))
    door = (j0 + j1)/2
    through_door = np.linalg.norm(a - door) + np.linalg.norm(b - door)
    assert np.isfinite(g) and g >= through_door - .3 and g <= 1.09*through_door + .3
    assert g > np.linalg.norm(a - b) + .5                                # (the straight line goes through the wall)
    # with the door shut the far room is out of reach: nothing leaks through the wall
    shut = np.concatenate([walls, np.array([[j0, j1]], F)])
    free_shut = nav_rule.free(shut, geom, CELL, RADIUS)
    D = nav_rule.field(free_shut, geom, CELL, b)
    assert np.isinf(nav_rule.query(D, geom, CELL, free_shut, a))
    assert np.isfinite(D).sum() > 500


def test_the_box_has_octile_distances():
    """toys.box(), goal at a cell centre: every free cell of the room holds the octile distance of its offset, to 64 half-ulps of 8 m."""
    from megastep_amd import toys
    walls = np.asarray(toys.box()['walls'], F)
    geom = nav_rule.geometry(walls, CELL)
    free = nav_rule.free(walls, geom, CELL, RADIUS)
    x, y = nav_rule.centres(geom, CELL)
    i0, j0 = free.shape[0]//2, free.shape[1]//2
    assert free[i0, j0]
    D = nav_rule.field(free, geom, CELL, (x[j0], y[i0]))
    assert D[i0, j0] == 0
    di, dj = np.abs(np.arange(free.shape[0]) - i0)[:, None], np.abs(np.arange(free.shape[1]) - j0)[None, :]
    octile = CELL*(np.maximum(di, dj) - np.minimum(di, dj)) + float(F(CELL)*DIAGONAL)*np.minimum(di, dj)
    lo, hi = walls.reshape(-1, 2).min(0), walls.reshape(-1, 2).max(0)
    room = free & ((x > lo[0]) & (x < hi[0]))[None, :] & ((y > lo[1]) & (y < hi[1]))[:, None]      # (the margin outside the walls is free too)
    assert room.sum() > 1000 and np.maximum(di, dj)[room].max() <= 64
    assert np.abs(D[room].astype(np.float64) - octile[room]).max() <= 64*2.**-21
    assert np.isinf(D[~room]).all()


def test_the_distance_is_never_shorter_than_the_straight_line():
    rng = np.random.RandomState(2)
    for g in plans(2) + plans(2, oblique=True):
        walls, geom, free = _world(g)
        pts = spawn_points(g)
        goal = pts[rng.randint(len(pts))]
        D = nav_rule.field(free, geom, CELL, goal)
        qs = pts[rng.choice(len(pts), 300)] + rng.uniform(-.05, .05, (300, 2)).astype(F)
        got = np.array([nav_rule.query(D, geom, CELL, free, q) for q in qs], np.float64)
        straight = np.linalg.norm(qs.astype(np.float64) - goal.astype(np.float64), axis=1)
        assert np.isfinite(got).sum() > 100
        assert (got >= straight - 1e-5).all()


def test_most_spawn_points_make_goals_worth_comparing():
    """The condition on the inputs that keeps the GPU tests' equality from being vacuous: of the spawn-table points of the plain
    and oblique plans they use, at least 90 % have an anchor and a finite region of more than 500 cells."""
    good = total = 0
    for g in plans(8) + plans(8, oblique=True):
        walls, geom, free = _world(g)
        u, v, _ = nav_rule.edges(free, CELL)
        label = np.arange(free.size)
        while True:                                                     # connected components by label propagation
            new = label.copy()
            np.minimum.at(new, v, label[u])
            new = new[new]
            if np.array_equal(new, label):
                break
            label = new
        size = np.bincount(label, minlength=free.size)
        for p in spawn_points(g):
            anchors = nav_rule.anchors(p, geom, CELL, free)
            total += 1
            good += bool(anchors) and max(size[label[i*free.shape[1] + j]] for i, j, _ in anchors) > 500
    assert total > 10000 and good >= .9*total, (good, total)


# ---------------------------------------------------------------------------------------------------------------------
# header, loader, refusals
# ---------------------------------------------------------------------------------------------------------------------
NAV_SYMBOLS = {'ms_nav_free', 'ms_nav_fields', 'ms_nav_query'}


def test_the_header_declares_the_nav_calls_and_the_loader_binds_them():
    from megastep_amd import _lib
    assert NAV_SYMBOLS <= set(declared_symbols(('megastep_hip.h',)))
    assert NAV_SYMBOLS <= set(_lib.SYMBOLS)
    text = open(os.path.join(ROOT, 'include', 'megastep_hip.h')).read()
    assert int(re.search(r'#define MS_ABI_VERSION (\d+)', text).group(1)) == _lib.ABI_VERSION == 17
    handle = _lib.lib()
    assert all(hasattr(handle, s) for s in NAV_SYMBOLS) and handle.ms_abi_version() == 17


@pytest.mark.parametrize('name,fields', [
    ('MsNavGrid', ('n_envs', 'cell', 'clearance', 'geom', 'starts', 'max_framed', 'free_cells')),
    ('MsNavFields', ('n_goals', 'goals', 'mask', 'fields', 'passes')),
    ('MsNavQuery', ('n_points', 'points', 'goal', 'fields', 'n_goals', 'out'))])
def test_the_nav_mirrors_have_the_c_layout(name, fields):
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


def test_bad_nav_arguments_are_refused_before_any_launch():
    from megastep_amd import _lib
    h = _lib.lib()
    fake = 64                                       # (never dereferenced: every call below fails its checks first)
    sc = _lib.MsScenery(n_envs=2, n_agents=1, n_model=8, lines_vals=64, lines_widths=64, lines_starts=64, model=64)
    grid = dict(n_envs=2, cell=.125, clearance=.106, geom=fake, starts=fake, max_framed=100, free_cells=fake)
    fields = dict(n_goals=1, goals=fake, mask=None, fields=fake, passes=None)
    query = dict(n_points=1, points=fake, goal=None, fields=fake, n_goals=1, out=fake)
    G, NF, NQ = _lib.MsNavGrid, _lib.MsNavFields, _lib.MsNavQuery
    ref = ctypes.byref
    assert h.ms_nav_free(None, ref(G(**grid)), None) == -1
    assert h.ms_nav_free(ref(sc), None, None) == -1
    assert h.ms_nav_fields(None, ref(NF(**fields)), None) == -1
    assert h.ms_nav_fields(ref(G(**grid)), None, None) == -1
    assert h.ms_nav_query(None, ref(NQ(**query)), None) == -1
    assert h.ms_nav_query(ref(G(**grid)), None, None) == -1
    assert h.ms_nav_free(ref(sc), ref(G(**{**grid, 'n_envs': 3})), None) == -1         # not the scenery's envs
    for bad in (dict(n_envs=0), dict(cell=0.), dict(cell=-1.), dict(cell=float('nan')), dict(cell=float('inf')), dict(clearance=0.),
                dict(clearance=float('nan')), dict(cell=.15), dict(cell=1.41*.106), dict(geom=None), dict(starts=None),
                dict(free_cells=None), dict(max_framed=-1), dict(geom=68)):
        g = G(**{**grid, **bad})
        assert h.ms_nav_free(ref(sc), ref(g), None) == -1, bad
        assert h.ms_nav_fields(ref(g), ref(NF(**fields)), None) == -1, bad
        assert h.ms_nav_query(ref(g), ref(NQ(**query)), None) == -1, bad
    for bad in (dict(n_goals=0), dict(n_goals=-2), dict(goals=None), dict(fields=None), dict(goals=68)):
        assert h.ms_nav_fields(ref(G(**grid)), ref(NF(**{**fields, **bad})), None) == -1, bad
    for bad in (dict(n_points=0), dict(n_goals=0), dict(points=None), dict(fields=None), dict(out=None), dict(n_points=2),
                dict(points=68)):
        assert h.ms_nav_query(ref(G(**grid)), ref(NQ(**{**query, **bad})), None) == -1, bad


def _cpu_scenery(n=3, n_agents=1, **kw):
    from megastep_amd import scene
    geoms = plans(n, **kw)
    return geoms, scene.scenery(geoms, n_agents, device='cpu', random=np.random.RandomState(0), bake=False)


def test_nav_geometry_is_the_rules_and_the_python_calls_refuse_what_they_cannot_do():
    from megastep_amd import cuda
    geoms, sc = _cpu_scenery(3)
    geom, starts = cuda.nav_geometry(sc, CELL)
    af = sc.n_agents*sc.model.shape[0]
    for e in range(3):
        walls = sc.lines[e][af:].numpy()
        assert tuple(geom[e]) == nav_rule.geometry(walls, CELL)
        x, y = nav_rule.centres(tuple(geom[e]), CELL)
        pts = walls.reshape(-1, 2)
        assert x[0] <= pts[:, 0].min() - CELL/2 and x[-1] > pts[:, 0].max() + CELL/2        # (a cell of margin: at least half a cell beyond the walls)
        assert y[0] <= pts[:, 1].min() - CELL/2 and y[-1] > pts[:, 1].max() + CELL/2
    assert starts[0] == 0 and np.array_equal(np.diff(starts), geom[:, 2].astype(np.int64)*geom[:, 3])
    with pytest.raises(RuntimeError, match='GPU'):
        cuda.nav_grid(sc, clearance=RADIUS)
    with pytest.raises(RuntimeError, match='1.4'):
        cuda.nav_grid(sc, cell=.2, clearance=RADIUS)
    with pytest.raises(RuntimeError, match='positive'):
        cuda.nav_grid(sc, cell=0., clearance=RADIUS)


@pytest.mark.parametrize('cell,r', CELLS)
def test_nav_geometry_is_the_rules_at_other_cell_widths(cell, r):
    """floor(x/c) of the walls' bounding box at cells that are no power of two, and the pairs pass nav_grid's own check (what is
    refused then is the CPU scenery)."""
    from megastep_amd import cuda
    geoms, sc = _cpu_scenery(3)
    geom, starts = cuda.nav_geometry(sc, cell)
    af = sc.n_agents*sc.model.shape[0]
    for e in range(3):
        walls = sc.lines[e][af:].numpy()
        assert tuple(geom[e]) == nav_rule.geometry(walls, cell)
        x, y = nav_rule.centres(tuple(geom[e]), cell)
        pts = walls.reshape(-1, 2)
        assert x[0] <= pts[:, 0].min() - cell/2 and x[-1] > pts[:, 0].max() + cell/2
        assert y[0] <= pts[:, 1].min() - cell/2 and y[-1] > pts[:, 1].max() + cell/2
    assert starts[0] == 0 and np.array_equal(np.diff(starts), geom[:, 2].astype(np.int64)*geom[:, 3])
    with pytest.raises(RuntimeError, match='GPU'):
        cuda.nav_grid(sc, cell=cell, clearance=r)


# ---------------------------------------------------------------------------------------------------------------------
# the envs' bookkeeping, against hand-filled fields
# ---------------------------------------------------------------------------------------------------------------------
def test_goals_take_the_first_reachable_candidate():
    from megastep_amd import modules
    inf = float('inf')
    dist = torch.tensor([[[inf, 3., 1.]], [[2., inf, inf]], [[inf, inf, inf]], [[inf, inf, 4.]]])       # (N=4, A=1, K=3)
    cand = torch.arange(4*3*2, dtype=torch.float32).reshape(4, 1, 3, 2)
    here = -torch.ones(4, 1, 2)
    goal, none = modules.Goals.choose(dist, cand, here)
    assert none.tolist() == [[False], [False], [True], [False]]
    assert torch.equal(goal[0, 0], cand[0, 0, 1]) and torch.equal(goal[1, 0], cand[1, 0, 0]) and torch.equal(goal[3, 0], cand[3, 0, 2])
    assert torch.equal(goal[2, 0], here[2, 0])                           # nowhere to go: the goal is where it stands


def test_pointgoal_books():
    from megastep_amd.demo.envs import pointgoal
    inf = float('inf')
    before = torch.tensor([[5.], [4.], [3.], [inf], [.6], [2.], [.3]])
    now = torch.tensor([[4.5], [4.25], [7.], [2.], [.4], [inf], [0.]])
    reset = torch.tensor([[False], [False], [True], [False], [False], [False], [False]])
    stranded = torch.tensor([[False], [False], [False], [False], [False], [True], [True]])
    reward, ended = pointgoal.books(before, now, reset, stranded, arrive=.5, bonus=10.)
    # progress; a step back; a reset step earns nothing; nor does a distance that was not finite; arrival; two stranded agents,
    # of which the second stands on its own goal and has not thereby arrived
    assert reward[:, 0].tolist() == [.5, -.25, 0., 0., pytest.approx(.2 + 10.), 0., pytest.approx(.3)]
    assert ended[:, 0].tolist() == [False, False, False, False, True, True, True]


class _Fields:
    """A hand-filled stand-in for cuda.DistanceFields: the distance to an agent's goal is the straight line, unless the goal is
    beyond x = 10, which nothing reaches."""

    def __init__(self, goals):
        self.goals = goals.clone()

    def update(self, goals=None, mask=None):
        if goals is not None:
            self.goals = torch.where(mask[..., None], goals, self.goals) if mask is not None else goals.clone()
        return self

    def at(self, points, goal=None, out=None):
        g = self.goals if goal is None else torch.gather(self.goals, 1, goal.long()[..., None].expand(-1, -1, 2))
        d = (points - g).norm(dim=-1)
        return torch.where((g[..., 0] > 10) | (points[..., 0] > 10), torch.full_like(d, float('inf')), d)


def test_goals_module_redraws_only_the_marked_agents_and_flags_the_stranded(monkeypatch):
    from megastep_amd import cuda, modules, core as core_mod
    geoms, sc = _cpu_scenery(4)
    c = core_mod.Core(sc, res=16)
    monkeypatch.setattr(cuda, 'distance_fields', lambda grid, goals, mask=None, out=None: _Fields(goals) if out is None else out.update(goals, mask))
    torch.manual_seed(0)
    table = torch.rand(4, 1, 20, 2)*8
    table[1] += 20.                                                     # env 1: every candidate out of reach
    table[2, :, :5] += 20.                                              # env 2: the first few are
    goals = modules.Goals(geoms, c, grid=object(), candidates=8, table=table)
    c.agents.positions[:] = torch.rand(4, 1, 2)*8
    goals(c.agent_full(True))
    assert goals.stranded[:, 0].tolist() == [False, True, False, False]
    assert torch.equal(goals.goals[1], c.agents.positions[1])
    d = goals.distances()
    assert d.shape == (4, 1) and torch.isfinite(d[[0, 2, 3]]).all() and d[1, 0] == 0
    assert (goals.goals[[0, 2, 3], 0, 0] <= 10).all()
    before = goals.goals.clone()
    mask = torch.tensor([[True], [False], [False], [False]])
    for _ in range(8):
        goals(mask)
    assert torch.equal(goals.goals[1:], before[1:])
    obs = goals.observation()
    assert obs.shape == (4, 1, 3) and goals.space.shape == (1, 3)
    off = goals.goals - c.agents.positions
    torch.testing.assert_close(obs[..., 2], off.norm(dim=-1))
    torch.testing.assert_close(obs[..., :2], modules.to_local_frame(c.agents.angles, off))
