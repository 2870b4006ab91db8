"""View fields (include/megastep_hip.h, MsNavViews) restated in numpy - view_rule, one binary32 operation a
statement - and the host instantiation of the kernel's own pieces (ms_host_nav_views: csrc/kernels/navview.h, through the kernel's
window, its wall cull and both of its wall paths) held to EQUALITY with it; the rule itself held to float64 geometry written
independently of it; hand-made worlds with known answers; the C-ABI's declarations, layout and refusals; the Python layer's
refusals and `BestViews.choose`. No GPU: what is compared is the text every lane of the kernel evaluates, swept serially."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests.test_abi import ROOT, declared_symbols
from tests.test_navfield_host import CELL, CELLS, RADIUS, F, _world, nav_rule, plans, spawn_points
from tests.test_navdraw_host import _aligned

NAN = F(np.nan)
CONE = 130.                                          # degrees, the cone of the cases that have one


def cos_half_of(fov):
    """What cuda.view_fields makes of ``fov`` degrees, on the host."""
    return float(np.cos(np.deg2rad(float(fov))/2.))


class view_rule:
    """The contract in numpy: every statement one binary32 operation, in the order the header gives."""

    @staticmethod
    def centres(geom, cell):
        x, y = nav_rule.centres(geom, cell)
        return np.broadcast_arrays(x[None, :], y[:, None])

    @staticmethod
    def in_range(geom, cell, p, R):
        """(ny, nx) bool: rr <= R2 (all False for a viewpoint that is not finite)."""
        x, y = view_rule.centres(geom, cell)
        px, py = F(p[0]), F(p[1])
        if not (np.isfinite(px) and np.isfinite(py)):
            return np.zeros(x.shape, bool)
        R2 = F(R)*F(R)
        rx = x - px
        ry = y - py
        a = rx*rx
        b = ry*ry
        rr = a + b
        return rr <= R2

    @staticmethod
    def in_cone(geom, cell, p, heading, cos_half):
        x, y = view_rule.centres(geom, cell)
        px, py, hx, hy = F(p[0]), F(p[1]), F(heading[0]), F(heading[1])
        with np.errstate(all='ignore'):
            a = hx*hx
            b = hy*hy
            hlen = np.sqrt(F(a + b))
            if not (np.isfinite(hlen) and hlen > 0):
                return np.zeros(x.shape, bool)
            rx = x - px
            ry = y - py
            a = rx*rx
            b = ry*ry
            rr = a + b
            length = np.sqrt(rr)
            a = hx*rx
            b = hy*ry
            dotp = a + b
            lim = F(cos_half)*length
            lim = lim*hlen
            return dotp >= lim

    @staticmethod
    def blocks(px, py, x, y, walls):
        """(cells, walls) bool: does wall w block the cell whose centre is (x, y) - meets, apart and across."""
        px, py = F(px), F(py)
        x, y = np.asarray(x, F)[:, None], np.asarray(y, F)[:, None]
        ax, ay, bx, by = (np.asarray(walls, F).reshape(-1, 4)[None, :, k] for k in range(4))
        with np.errstate(invalid='ignore', over='ignore'):
            meets = (np.minimum(ax, bx) <= np.maximum(px, x)) & (np.maximum(ax, bx) >= np.minimum(px, x)) & \
                    (np.minimum(ay, by) <= np.maximum(py, y)) & (np.maximum(ay, by) >= np.minimum(py, y))
            rx = x - px
            ry = y - py
            vx = bx - ax
            vy = by - ay
            s = py - ay
            t = px - ax
            m = vx*s
            n = vy*t
            o1 = m - n
            s = y - ay
            t = x - ax
            m = vx*s
            n = vy*t
            o2 = m - n
            apart = ((o1 < 0) & (o2 > 0)) | ((o1 > 0) & (o2 < 0))
            s = ay - py
            t = ax - px
            m = rx*s
            n = ry*t
            o3 = m - n
            s = by - py
            t = bx - px
            m = rx*s
            n = ry*t
            o4 = m - n
            across = ((o3 <= 0) & (o4 >= 0)) | ((o3 >= 0) & (o4 <= 0))
        return meets & apart & across

    @staticmethod
    def visible(walls, geom, cell, p, R, heading=None, cos_half=None):
        """(ny, nx) bool: the cells in sight of p."""
        ok = view_rule.in_range(geom, cell, p, R)
        if heading is not None:
            ok = ok & view_rule.in_cone(geom, cell, p, heading, cos_half)
        walls = np.asarray(walls, F).reshape(-1, 4)
        if ok.any() and len(walls):
            x, y = view_rule.centres(geom, cell)
            i, j = np.nonzero(ok)
            blocked = np.zeros(len(i), bool)
            for at in range(0, len(walls), 64):
                blocked |= view_rule.blocks(p[0], p[1], x[i, j], y[i, j], walls[at:at + 64]).any(1)
            ok = ok.copy()
            ok[i, j] = ~blocked
        return ok

    @staticmethod
    def slot_of(S, P, slot, n, p):
        s = int(slot[n][p]) if slot is not None else (0 if S == 1 else p)
        return s if 0 <= s < S else -1

    @staticmethod
    def call(geom, starts, cell, walls, points, R, countable, headings=None, cos_half=None, unseen=None, S=0, slot=None, mask=None,
             before=None, images=None):
        """One call of ms_nav_views: dict of values (flat, the seen maps' layout), counts and gains (N, P); `walls`: a list of
        (L, 4) per env; `before`: what the outputs held (masked-out viewpoints keep it); `images`: {(n, p): visible} known already."""
        N, P = points.shape[:2]
        size = max(P*int(starts[-1]), 1)
        out = before if before is not None else dict(values=np.zeros(size, np.uint8), counts=np.zeros((N, P), np.int32), gains=np.zeros((N, P), np.int32))
        out = {k: np.array(v) for k, v in out.items()}
        for n in range(N):
            nx, ny = int(geom[n][2]), int(geom[n][3])
            n_cells = nx*ny if nx > 0 and ny > 0 else 0
            first = int(starts[n])
            for p in range(P):
                if mask is not None and not mask[n][p]:
                    continue
                out['counts'][n, p] = out['gains'][n, p] = 0
                if n_cells == 0:
                    continue
                if images is not None and (n, p) in images:
                    vis = images[n, p]
                else:
                    vis = view_rule.visible(walls[n], tuple(int(v) for v in geom[n]), cell, points[n, p], R,
                                            None if headings is None else headings[n, p], cos_half)
                vis = vis.reshape(-1)
                out['values'][P*first + p*n_cells:][:n_cells] = vis
                counted = vis & ((np.asarray(countable)[first:first + n_cells] & 1) != 0)
                out['counts'][n, p] = counted.sum()
                s = view_rule.slot_of(S, P, slot, n, p) if unseen is not None else -1
                if s >= 0:
                    out['gains'][n, p] = (counted & ((np.asarray(unseen)[S*first + s*n_cells:][:n_cells] & 1) == 0)).sum()
        return out


# ---------------------------------------------------------------------------------------------------------------------
# the host instantiation
# ---------------------------------------------------------------------------------------------------------------------
def _max_framed(geom):
    framed = [(int(g[2]) + 2)*(int(g[3]) + 2) for g in geom if g[2] > 0 and g[3] > 0]
    return max(framed, default=0)


class _Host:
    """ms_host_nav_views on one grid of host arrays; the outputs start as sentinels."""

    def __init__(self, geom, starts, free, walls, cell=CELL, clearance=RADIUS):
        from megastep_amd import _lib
        self.geom, self.starts = _aligned(geom), np.ascontiguousarray(starts, np.int64)
        self.free = np.ascontiguousarray(np.concatenate([np.asarray(free, np.uint8).reshape(-1), np.zeros(1, np.uint8)]))
        self.N, self.cell = len(self.geom), cell
        self.walls = np.ascontiguousarray(np.concatenate([np.asarray(w, F).reshape(-1, 4) for w in walls] + [np.zeros((1, 4), F)]))
        self.wall_starts = np.concatenate([[0], np.cumsum([len(np.asarray(w).reshape(-1, 4)) for w in walls])]).astype(np.int64)
        self.grid = _lib.MsNavGrid(self.N, cell, clearance, self.geom.ctypes.data, self.starts.ctypes.data, _max_framed(self.geom), self.free.ctypes.data)
        self.h = _lib.lib()

    def views(self, points, R, countable, headings=None, cos_half=0., unseen=None, S=0, slot=None, mask=None, before=None, capacity=0,
              store=True, expect=0):
        from megastep_amd import _lib
        points = np.ascontiguousarray(points, F)
        N, P = points.shape[:2]
        size = max(P*int(self.starts[-1]), 1)
        out = before if before is not None else dict(values=np.full(size, 9, np.uint8), counts=np.full((N, P), -7, np.int32), gains=np.full((N, P), -7, np.int32))
        out = {k: np.ascontiguousarray(v).copy() for k, v in out.items()}
        keep = [None if a is None else np.ascontiguousarray(a, t) for a, t in
                ((headings, F), (countable, np.uint8), (unseen, np.uint8), (slot, np.int32), (mask, np.uint8))]
        ptr = lambda a: None if a is None else a.ctypes.data
        spec = _lib.MsNavViews(P, points.ctypes.data, ptr(keep[0]), float(R), float(cos_half), ptr(keep[1]), ptr(keep[2]), S, ptr(keep[3]), ptr(keep[4]),
                               out['values'].ctypes.data if store else None, out['counts'].ctypes.data,
                               out['gains'].ctypes.data if unseen is not None else None)
        status = self.h.ms_host_nav_views(ctypes.byref(self.grid), ctypes.byref(spec), self.walls.ctypes.data, self.wall_starts.ctypes.data, capacity)
        assert status == expect
        return out


def same(got, want, keys=('values', 'counts', 'gains')):
    for key in keys:
        assert np.array_equal(got[key], want[key]), (key, int((np.asarray(got[key]) != np.asarray(want[key])).sum()))


def wall_distance(p, walls):
    """The least float64 distance from p to the segments `walls` (L, 4)."""
    w = np.asarray(walls, np.float64).reshape(-1, 4)
    a, v = w[:, :2], w[:, 2:] - w[:, :2]
    q = np.asarray(p, np.float64)[None] - a
    t = np.clip((q*v).sum(1)/np.maximum((v*v).sum(1), 1e-300), 0., 1.)
    return float(np.sqrt(((q - t[:, None]*v)**2).sum(1)).min())


class _Plans:
    pass


_PLANS = {}


def plan_views(cell=CELL, r=RADIUS, ranges=(4., 10.)):
    """The six plans as one ragged grid with two viewpoints a plan (the issue's draw), the rule's images for R in {4, 10} with and
    without the cone, a random half-seen pair of maps an env, and the host on it."""
    if (cell, r) not in _PLANS:
        w = _Plans()
        w.cell = cell
        gs = plans(3) + plans(3, oblique=True)
        worlds = [_world(g, cell, r) for g in gs]
        w.walls = [np.asarray(walls, F).reshape(-1, 4) for walls, _, _ in worlds]
        w.geom = np.array([geom for _, geom, _ in worlds], np.int32)
        w.images = [free for _, _, free in worlds]
        w.starts = np.concatenate([[0], np.cumsum([f.size for f in w.images])]).astype(np.int64)
        w.free = np.concatenate([f.reshape(-1) for f in w.images]).astype(np.uint8)
        rng = np.random.RandomState(5)
        w.points = np.full((6, 2, 2), NAN, F)
        for n, g in enumerate(gs):
            sp = spawn_points(g)
            for p in range(2):
                for _ in range(50):
                    cand = (sp[rng.choice(len(sp))] + rng.uniform(-.05, .05, 2)).astype(F)
                    if wall_distance(cand, w.walls[n]) >= r:
                        w.points[n, p] = cand
                        break
        assert np.isfinite(w.points).all()
        heads = np.random.RandomState(11).uniform(-1, 1, (6, 2, 2))
        w.headings = (heads*np.array([.5, 3.])[None, :, None]).astype(F)        # (any length: the rule scales by it)
        w.cos_half = cos_half_of(CONE)
        w.seen = (np.random.RandomState(12).rand(2*len(w.free)) < .5).astype(np.uint8)*np.random.RandomState(13).choice(np.array([1, 3], np.uint8), 2*len(w.free))
        w.vis = {}
        for R in ranges:
            for cone in (False, True):
                w.vis[R, cone] = {(n, p): view_rule.visible(w.walls[n], tuple(int(v) for v in w.geom[n]), cell, w.points[n, p], R,
                                                            w.headings[n, p] if cone else None, w.cos_half if cone else None)
                                  for n in range(6) for p in range(2)}
        w.host = _Host(w.geom, w.starts, w.free, w.walls, cell, r)
        _PLANS[cell, r] = w
    return _PLANS[cell, r]


@pytest.mark.parametrize('capacity', [0, 8])
@pytest.mark.parametrize('cone', [False, True])
@pytest.mark.parametrize('R', [4., 10.])
def test_the_host_instantiation_is_the_rule_on_the_six_plans(R, cone, capacity):
    """Bytes, counts and gains (P = 2 against S = 2), staged walls and - with 8 rows of room - the sweep over all of them."""
    _host_is_the_rule_on_the_six_plans(plan_views(), R, cone, capacity)


@pytest.mark.parametrize('cell,r', CELLS)
@pytest.mark.parametrize('cone', [False, True])
def test_the_host_instantiation_is_the_rule_at_other_cell_widths(cone, cell, r):
    """The same walls, viewpoints and headings over grids whose cell is no power of two, at a range of 4 m, through both wall paths:
    the window of cells a viewpoint sweeps rests on rounded quotients there, and every cell in range must still be in it. Every
    viewpoint has visible and hidden free cells."""
    w = plan_views(cell, r, ranges=(4.,))
    for image, (n, p) in ((w.vis[4., cone][n, p], (n, p)) for n in range(6) for p in range(2)):
        assert (image & w.images[n]).any() and (~image & w.images[n]).any(), (n, p)
    for capacity in (0, 8):
        _host_is_the_rule_on_the_six_plans(w, 4., cone, capacity)


def _host_is_the_rule_on_the_six_plans(w, R, cone, capacity):
    kw = dict(headings=w.headings, cos_half=w.cos_half) if cone else {}
    got = w.host.views(w.points, R, w.free, unseen=w.seen, S=2, capacity=capacity, **kw)
    want = view_rule.call(w.geom, w.starts, w.cell, w.walls, w.points, R, w.free, unseen=w.seen, S=2, images=w.vis[R, cone], **kw)
    same(got, want)
    assert (want['counts'] > 0).all() and (want['gains'] <= want['counts']).all() and 0 < want['gains'].sum() < want['counts'].sum()
    if capacity:                                     # (every viewpoint keeps more rows than that: the other wall path)
        for n in range(6):
            lo, hi = np.minimum(w.walls[n][:, :2], w.walls[n][:, 2:]), np.maximum(w.walls[n][:, :2], w.walls[n][:, 2:])
            for p in range(2):
                assert ((lo <= w.points[n, p] + R) & (hi >= w.points[n, p] - R)).all(1).sum() > capacity
    # without a byte store the same counts and gains, and no byte written
    bare = w.host.views(w.points, R, w.free, unseen=w.seen, S=2, capacity=capacity, store=False, **kw)
    same(bare, want, ('counts', 'gains'))
    assert (bare['values'] == 9).all()


def test_one_map_an_env_a_slot_and_a_mask_on_the_six_plans():
    w = plan_views()
    R = 4.
    one = w.seen.reshape(-1)[:len(w.free)]                                # (S = 1: both viewpoints against the env's one map)
    got = w.host.views(w.points, R, w.free, unseen=one, S=1)
    same(got, view_rule.call(w.geom, w.starts, CELL, w.walls, w.points, R, w.free, unseen=one, S=1, images=w.vis[R, False]))
    slot = np.array([[1, 0], [0, 0], [1, 1], [2, 0], [0, -1], [1, 0]], np.int32)
    mask = np.array([[1, 1], [0, 1], [1, 0], [1, 1], [1, 1], [0, 0]], np.uint8)
    countable = (w.free*(np.random.RandomState(3).rand(len(w.free)) < .8)).astype(np.uint8)*3
    before = dict(values=np.full(2*len(w.free), 9, np.uint8), counts=np.full((6, 2), -7, np.int32), gains=np.full((6, 2), -7, np.int32))
    got = w.host.views(w.points, R, countable, unseen=w.seen, S=2, slot=slot, mask=mask, before=before)
    want = view_rule.call(w.geom, w.starts, CELL, w.walls, w.points, R, countable, unseen=w.seen, S=2, slot=slot, mask=mask, before=before,
                          images=w.vis[R, False])
    same(got, want)
    assert got['gains'][3, 0] == 0 and got['gains'][4, 1] == 0 and got['counts'][3, 0] > 0        # (a slot outside 0 .. S - 1 gives 0)
    assert got['counts'][1, 0] == -7 and got['gains'][5, 1] == -7
    at = 2*int(w.starts[1])
    assert (got['values'][at:at + w.images[1].size] == 9).all()            # (a masked-out viewpoint keeps its bytes)


def test_the_cases_see_and_hide_enough_for_the_equality_to_mean_something():
    w = plan_views()
    seen, hidden, in_range = [], [], []
    for R in (4., 10.):
        for n in range(6):
            for p in range(2):
                near = view_rule.in_range(tuple(int(v) for v in w.geom[n]), CELL, w.points[n, p], R) & w.images[n]
                vis = w.vis[R, False][n, p] & w.images[n]
                seen.append(int(vis.sum())); hidden.append(int((near & ~vis).sum())); in_range.append(int(near.sum()))
    print('least seen', min(seen), 'least hidden', min(hidden), 'visible', sum(seen), 'of', sum(in_range), 'in-range free cells')
    assert min(seen) >= 200 and min(hidden) >= 200


def _crossings(p, centres, walls, lo, hi):
    """(cells,) bool in float64, written apart from the rule: does the open segment p -> centre cross some wall at a wall
    parameter in [lo, hi] - p + t r = a + u v with t in (0, 1)."""
    p = np.asarray(p, np.float64)
    r = np.asarray(centres, np.float64) - p                                # (cells, 2)
    w = np.asarray(walls, np.float64).reshape(-1, 4)
    a, v = w[:, :2], w[:, 2:] - w[:, :2]
    q = a - p                                                              # (walls, 2)
    denom = r[:, None, 0]*v[None, :, 1] - r[:, None, 1]*v[None, :, 0]
    with np.errstate(divide='ignore', invalid='ignore'):
        t = (q[None, :, 0]*v[None, :, 1] - q[None, :, 1]*v[None, :, 0])/denom
        u = (q[None, :, 0]*r[:, None, 1] - q[None, :, 1]*r[:, None, 0])/denom
        hit = (denom != 0) & (t > 0) & (t < 1) & (u >= lo) & (u <= hi)
    return hit.any(1)


def test_no_wall_is_seen_through_and_nothing_in_plain_sight_is_hidden():
    w = plan_views()
    through = spurious = 0
    for R in (4., 10.):
        for n in range(6):
            geom = tuple(int(v) for v in w.geom[n])
            x, y = view_rule.centres(geom, CELL)
            for p in range(2):
                near = view_rule.in_range(geom, CELL, w.points[n, p], R) & w.images[n]
                vis = w.vis[R, False][n, p]
                i, j = np.nonzero(near & vis)
                through += int(_crossings(w.points[n, p], np.stack([x[i, j], y[i, j]], -1), w.walls[n], 1e-6, 1 - 1e-6).sum())
                i, j = np.nonzero(near & ~vis)
                spurious += int((~_crossings(w.points[n, p], np.stack([x[i, j], y[i, j]], -1), w.walls[n], -1e-6, 1 + 1e-6)).sum())
    assert through == 0 and spurious == 0


# ---------------------------------------------------------------------------------------------------------------------
# hand-made worlds
# ---------------------------------------------------------------------------------------------------------------------
def box_walls(nan_row=True):
    """An 8 x 4 box, a partition at x = 4 with a door from y = 1.5 to 2.5, and a row of NaN."""
    rows = [(0, 0, 8, 0), (8, 0, 8, 4), (8, 4, 0, 4), (0, 4, 0, 0), (4, 0, 4, 1.5), (4, 2.5, 4, 4)]
    if nan_row:
        rows.insert(3, (np.nan, 1, 3, np.nan))
    return np.array(rows, F)


def centre_of(geom, i, j):
    return np.array([(F(geom[0] + j) + F(.5))*F(CELL), (F(geom[1] + i) + F(.5))*F(CELL)], F)


class _Hand:
    pass


_HAND = []


def hand():
    """Five envs, eight viewpoints each. 0: the box (see box_walls); 1: two walls that share the vertex (1, 1), and nothing else;
    2: no cells; 3: cells and no static wall; 4: a few oblique walls."""
    if not _HAND:
        w = _Hand()
        rng = np.random.RandomState(21)
        vertex = np.array([(1, 1, 0, 2), (1, 1, 2, 0)], F)
        oblique = np.concatenate([rng.uniform(0, 5, (9, 4)), [[0, 0, 5, 0], [5, 0, 5, 5], [5, 5, 0, 5], [0, 5, 0, 0]]]).astype(F)
        w.walls = [box_walls(), vertex, np.zeros((0, 4), F), np.zeros((0, 4), F), oblique]
        w.geom = np.array([nav_rule.geometry(box_walls(False), CELL), nav_rule.geometry(vertex, CELL), (3, 4, 0, 7), (-10, 5, 40, 24),
                           nav_rule.geometry(oblique, CELL)], np.int32)
        w.images = [nav_rule.free(w.walls[n], tuple(int(v) for v in w.geom[n]), CELL, RADIUS) if w.geom[n][2] > 0 else np.zeros((7, 0), bool)
                    for n in range(5)]
        w.starts = np.concatenate([[0], np.cumsum([m.size for m in w.images])]).astype(np.int64)
        w.free = np.concatenate([m.reshape(-1) for m in w.images]).astype(np.uint8)
        w.free[w.free != 0] = rng.choice(np.array([1, 3, 255], np.uint8), int((w.free != 0).sum()))       # (bit 0 is what counts)
        g0, g3 = w.geom[0], w.geom[3]
        w.on_centre = centre_of(g0, 12, 20)
        pts = np.empty((5, 8, 2), F)
        pts[0] = [(1, 2), (4, 2), w.on_centre, (-3, 2), (np.nan, 1), (.3, .3), (7.8, 3.8), (6, 1)]
        pts[1] = [(.6875, .6875), (1.3125, 1.3125), (.5, 1.9), (1.9, .4), (1, np.inf), (0, 0), (2.2, 2.2), (-.1, 1)]
        pts[2] = rng.uniform(0, 1, (8, 2))
        pts[3] = [centre_of(g3, 0, 0), centre_of(g3, 23, 39), (0, 2), (-1.3, .7), (3.6, 3.5), (1.2, 50), (-9, 1), (1.234, 1.111)]
        pts[4] = rng.uniform(-.3, 5.3, (8, 2))
        w.points = pts
        heads = rng.uniform(-1, 1, (5, 8, 2)).astype(F)
        heads[0, 0] = (0, 0)                                               # (a zero heading sees nothing)
        heads[3, 2] = (np.nan, 1)
        heads[4, 1] = (0, -0.)
        w.headings = heads
        w.seen = (rng.rand(8*len(w.free)) < .4).astype(np.uint8)
        w.host = _Host(w.geom, w.starts, w.free, w.walls)
        _HAND.append(w)
    return _HAND[0]


def _hand_call(w, R, cone=False, capacity=0):
    kw = dict(headings=w.headings, cos_half=cos_half_of(CONE)) if cone else {}
    got = w.host.views(w.points, R, w.free, unseen=w.seen, S=8, capacity=capacity, **kw)
    want = view_rule.call(w.geom, w.starts, CELL, w.walls, w.points, R, w.free, unseen=w.seen, S=8, **kw)
    same(got, want)
    return want


def _store(w, out, n, p, P=8):
    size = w.images[n].size
    return out['values'][P*int(w.starts[n]) + p*size:][:size].reshape(w.images[n].shape).astype(bool)


@pytest.mark.parametrize('capacity', [0, 3])
def test_the_hand_made_worlds_with_everything_in_range(capacity):
    """R = 20: the box's far room through the door, a viewpoint on a cell centre, on a wall's line, outside the grid, a NaN one;
    the shared vertex; no cells; no walls; with room for three rows - more kept walls than fit - the same bytes. At a cell of
    0.125 only: the hand-made viewpoints and the cells named below are written out for it."""
    w = hand()
    want = _hand_call(w, 20., capacity=capacity)
    g0 = tuple(int(v) for v in w.geom[0])
    x, y = (a.astype(np.float64) for a in view_rule.centres(g0, CELL))
    inside = (x > 0) & (x < 8) & (y > 0) & (y < 4)
    # from (1, 2) the near room is in sight; the far room where the sight line passes the door, and nowhere else
    vis = _store(w, want, 0, 0)
    at_door = 2. + (y - 2.)*(4. - 1.)/np.where(x > 4, x - 1., 1.)
    far = inside & (x > 4)
    assert vis[inside & (x < 4)].all()
    assert vis[far & (at_door > 1.5 + 1e-6) & (at_door < 2.5 - 1e-6)].all() and not vis[far & ((at_door < 1.5 - 1e-6) | (at_door > 2.5 + 1e-6))].any()
    assert vis[far].any() and not vis[far].all() and not vis[~inside].any()
    # (4, 2) is on the partition's line: o1 == 0, the partition does not block, both rooms are in sight
    assert np.array_equal(_store(w, want, 0, 1), inside)
    # a viewpoint exactly on a cell's centre sees that cell
    assert _store(w, want, 0, 2)[12, 20] and (view_rule.centres(g0, CELL)[0][12, 20], view_rule.centres(g0, CELL)[1][12, 20]) == tuple(w.on_centre)
    # from outside the grid nothing inside the box; a NaN viewpoint sees nothing, its store written 0
    out = _store(w, want, 0, 3)
    assert out.any() and not out[inside].any()
    assert not _store(w, want, 0, 4).any() and want['counts'][0, 4] == 0 and want['gains'][0, 4] == 0
    # the sight line from (.6875, .6875) to the centre (1.3125, 1.3125) passes exactly through the vertex (1, 1): blocked
    g1 = tuple(int(v) for v in w.geom[1])
    j, i = int(round(1.3125/CELL - .5)) - g1[0], int(round(1.3125/CELL - .5)) - g1[1]
    assert tuple(centre_of(g1, i, j)) == (F(1.3125), F(1.3125))
    assert not _store(w, want, 1, 0)[i, j]
    each = view_rule.blocks(.6875, .6875, [F(1.3125)], [F(1.3125)], w.walls[1])
    assert each.all()                                                      # (by either wall, each with o3 == 0)
    assert _store(w, want, 1, 0)[i - 6, j - 6]                             # (and short of the walls it is not)
    # no cells: zeros, nothing stored; no walls: in range is in sight
    assert (want['counts'][2] == 0).all() and (want['gains'][2] == 0).all()
    g3 = tuple(int(v) for v in w.geom[3])
    for p in range(8):
        assert np.array_equal(_store(w, want, 3, p), view_rule.in_range(g3, CELL, w.points[3, p], 20.))
    assert _store(w, want, 3, 0).all() and not _store(w, want, 3, 5).any()


@pytest.mark.parametrize('R', [2., .75])
@pytest.mark.parametrize('cone', [False, True])
def test_windows_clipped_by_every_edge_and_odd_headings(R, cone):
    """Viewpoints by the left, bottom, top and right edges of their grids, on a corner cell and beyond the grid."""
    w = hand()
    want = _hand_call(w, R, cone)
    _hand_call(w, R, cone, capacity=2)
    if cone:
        assert want['counts'][0, 0] == 0 and want['counts'][3, 2] == 0 and want['counts'][4, 1] == 0 and not _store(w, want, 0, 0).any()
    else:
        assert _store(w, want, 3, 0)[0, 0] and _store(w, want, 3, 1)[23, 39] and want['counts'][0, 5] > 0 and want['counts'][0, 6] > 0


def test_a_range_below_half_a_cell_sees_the_cell_it_stands_on_or_nothing():
    """At a cell of 0.125 only: the range, the viewpoints and the cells named below are written out for it."""
    w = hand()
    want = _hand_call(w, .05)
    assert _store(w, want, 0, 2).sum() == 1 and _store(w, want, 0, 2)[12, 20] and _store(w, want, 3, 0).sum() == 1
    assert _store(w, want, 3, 1).sum() == 1 and not _store(w, want, 0, 0).any() and not _store(w, want, 3, 7).any()


# ---------------------------------------------------------------------------------------------------------------------
# header, loader, refusals
# ---------------------------------------------------------------------------------------------------------------------
FIELDS = ('n_points', 'points', 'headings', 'max_range', 'cos_half', 'countable', 'unseen', 'n_maps', 'slot', 'mask', 'values', 'counts', 'gains')


def test_the_header_declares_the_call_and_the_abi_version_stays():
    from megastep_amd import _lib, cuda
    assert 'ms_nav_views' in declared_symbols(('megastep_hip.h',))
    assert {'ms_host_nav_views', 'ms_host_nav_view_capacity'} <= set(declared_symbols(('megastep_hip_test.h',)))
    assert {'ms_nav_views', 'ms_host_nav_views', 'ms_host_nav_view_capacity'} <= set(_lib.SYMBOLS)
    text = open(os.path.join(ROOT, 'include', 'megastep_hip.h')).read()
    assert int(re.search(r'#define MS_ABI_VERSION (\d+)', text).group(1)) == _lib.ABI_VERSION == 17
    handle = _lib.lib()
    assert all(hasattr(handle, name) for name in ('ms_nav_views', 'ms_host_nav_views', 'ms_host_nav_view_capacity'))
    assert handle.ms_host_nav_view_capacity() == cuda.VIEW_WALL_CAPACITY


def test_the_mirror_has_the_c_layout():
    import subprocess
    import tempfile
    from megastep_amd import _lib
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "megastep_hip.h"\nint main(){printf("%zu", sizeof(MsNavViews));' +
           ''.join(f'printf(" %zu", offsetof(MsNavViews, {f}));' for f in FIELDS) + '}')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, 't.c'), 'w').write(src)
        subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), os.path.join(d, 't.c'), '-o', os.path.join(d, 't')])
        got = list(map(int, subprocess.check_output([os.path.join(d, 't')]).split()))
    assert [f for f, _ in _lib.MsNavViews._fields_] == list(FIELDS)
    assert got == [ctypes.sizeof(_lib.MsNavViews)] + [getattr(_lib.MsNavViews, f).offset for f in FIELDS]


def test_bad_arguments_are_refused_before_any_launch():
    from megastep_amd import _lib
    h = _lib.lib()
    fake = 64                                       # (never dereferenced: every call below fails its checks first)
    grid = _lib.MsNavGrid(n_envs=2, cell=.125, clearance=.106, geom=fake, starts=fake, max_framed=100, free_cells=fake)
    scenery = _lib.MsScenery(n_envs=2, n_agents=1, n_model=1, lines_vals=fake, lines_widths=fake, lines_starts=fake, model=fake)
    ref = ctypes.byref
    good = dict(n_points=2, points=fake, headings=fake, max_range=10., cos_half=.5, countable=fake, unseen=fake, n_maps=2, slot=None, mask=None,
                values=fake, counts=fake, gains=fake)
    bad_ones = (dict(n_points=0), dict(n_points=-1), dict(points=None), dict(countable=None), dict(values=None, counts=None, gains=None),
                dict(max_range=0.), dict(max_range=-1.), dict(max_range=float('inf')), dict(max_range=float('nan')),
                dict(cos_half=1.5), dict(cos_half=-1.01), dict(cos_half=float('nan')), dict(unseen=None), dict(n_maps=0), dict(n_maps=-2),
                dict(gains=None, n_maps=0), dict(n_maps=3), dict(points=68), dict(headings=68), dict(slot=66), dict(counts=66), dict(gains=66))
    for bad in bad_ones:
        spec = _lib.MsNavViews(**{**good, **bad})
        assert h.ms_nav_views(ref(scenery), ref(grid), ref(spec), None) == -1, bad
        assert h.ms_host_nav_views(ref(grid), ref(spec), fake, fake, 0) == -1, bad
    spec = _lib.MsNavViews(**good)
    assert h.ms_nav_views(None, ref(grid), ref(spec), None) == -1 and h.ms_nav_views(ref(scenery), None, ref(spec), None) == -1
    assert h.ms_nav_views(ref(scenery), ref(grid), None, None) == -1 and h.ms_host_nav_views(ref(grid), None, fake, fake, 0) == -1
    other = _lib.MsScenery(n_envs=3, n_agents=1, n_model=1, lines_vals=fake, lines_widths=fake, lines_starts=fake, model=fake)
    assert h.ms_nav_views(ref(other), ref(grid), ref(spec), None) == -1                 # (a scenery of another number of envs)
    assert h.ms_host_nav_views(ref(grid), ref(spec), None, fake, 0) == -1 and h.ms_host_nav_views(ref(grid), ref(spec), fake, None, 0) == -1
    assert h.ms_host_nav_views(ref(grid), ref(spec), fake, fake, h.ms_host_nav_view_capacity() + 1) == -1
    # a cone's cosine is not looked at without headings; an unseen store may go without gains
    w = hand()
    out = w.host.views(w.points, 1., w.free, cos_half=7.)
    same(out, view_rule.call(w.geom, w.starts, CELL, w.walls, w.points, 1., w.free), ('values', 'counts'))


def test_the_python_calls_refuse_what_they_cannot_do():
    from megastep_amd import cuda, nav, scene, toys
    assert cuda.view_fields is nav.view_fields and cuda.ViewFields is nav.ViewFields and cuda.VIEW_WALL_CAPACITY is nav.VIEW_WALL_CAPACITY
    geom = np.array([[0, 0, 8, 8], [0, 0, 8, 8]], np.int32)
    starts = np.array([0, 64, 128], np.int64)
    grid = cuda.NavGrid(torch.as_tensor(geom), torch.as_tensor(starts), torch.ones(128, dtype=torch.uint8), CELL, RADIUS, geom, starts)
    scenery = scene.scenery([toys.box(), toys.box()], 1, device='cpu', bake=False)
    points = torch.zeros((2, 3, 2))
    with pytest.raises(RuntimeError, match='GPU'):
        cuda.view_fields(grid, scenery, points)      # (CPU tensors)
    for bad in (torch.zeros((3, 3, 2)), torch.zeros((2, 3, 3)), torch.zeros((2, 0, 2))):
        with pytest.raises(RuntimeError, match=r'\(N, P, 2\)'):
            cuda.view_fields(grid, scenery, bad)
    with pytest.raises(RuntimeError):
        cuda.view_fields(grid, scenery, points.double())
    for bad in (0, -1., float('inf'), float('nan'), 'far'):
        with pytest.raises(RuntimeError, match='max_range'):
            cuda.view_fields(grid, scenery, points, max_range=bad)
    for kw in (dict(headings=points), dict(fov=90.)):
        with pytest.raises(RuntimeError, match='go together'):
            cuda.view_fields(grid, scenery, points, **kw)
    with pytest.raises(RuntimeError, match='headings must be'):
        cuda.view_fields(grid, scenery, points, headings=torch.zeros((2, 2, 2)), fov=90.)
    for bad in (-1., 361., float('nan'), None.__class__):
        with pytest.raises(RuntimeError, match='fov'):
            cuda.view_fields(grid, scenery, points, headings=points, fov=bad)
    with pytest.raises(RuntimeError, match='SeenMaps'):
        cuda.view_fields(grid, scenery, points, unseen=torch.zeros(128, dtype=torch.uint8))
    maps = cuda.seen_maps(grid, 2)
    with pytest.raises(RuntimeError, match='one per viewpoint'):
        cuda.view_fields(grid, scenery, points, unseen=maps)
    other = cuda.NavGrid(torch.as_tensor(geom), torch.as_tensor(starts), torch.ones(128, dtype=torch.uint8), CELL, RADIUS, geom, starts)
    with pytest.raises(RuntimeError, match='same grid'):
        cuda.view_fields(grid, scenery, points, unseen=cuda.seen_maps(other, 3))
    with pytest.raises(RuntimeError, match='slot goes with unseen'):
        cuda.view_fields(grid, scenery, points, slot=torch.zeros((2, 3), dtype=torch.int32))
    for bad in (torch.zeros((2, 3)), torch.zeros((2, 2), dtype=torch.int32), torch.zeros((2, 3), dtype=torch.bool)):
        with pytest.raises(RuntimeError, match='slot must be'):
            cuda.view_fields(grid, scenery, points, unseen=maps, slot=bad)
    for bad in (torch.ones(100, dtype=torch.uint8), torch.ones(128), torch.ones((2, 64), dtype=torch.uint8)):
        with pytest.raises(RuntimeError, match='countable'):
            cuda.view_fields(grid, scenery, points, countable=bad)
    with pytest.raises(RuntimeError, match='scenery'):
        cuda.view_fields(grid, scene.scenery([toys.box()], 1, device='cpu', bake=False), points)
    with pytest.raises(RuntimeError, match='GPU'):
        cuda.view_fields(grid, scenery, points, unseen=maps, slot=torch.zeros((2, 3), dtype=torch.int64))
    new = lambda shape, dtype: torch.zeros(shape, dtype=dtype)
    v = cuda.ViewFields(grid, scenery, points, 10., None, 0., grid.free, None, None, new(3*128, torch.uint8), new((2, 3), torch.int32), None)
    assert v.n_points == 3 and v.image(1, 2).shape == (8, 8) and v.image(1, 2).dtype == torch.bool
    for kw in (dict(points=torch.zeros((2, 2, 2))), dict(store=False), dict(unseen=cuda.seen_maps(grid, 3)), dict(grid=other)):
        kw = {**dict(grid=grid, points=points), **kw}
        with pytest.raises(RuntimeError, match='`out` must come from a view_fields call'):
            cuda.view_fields(kw.pop('grid'), scenery, **kw, out=v)
    with pytest.raises(RuntimeError, match='`out` must come from a view_fields call'):
        cuda.view_fields(grid, scenery, points, out=maps)
    for bad in (torch.ones((2, 3)), torch.ones((2, 2), dtype=torch.bool), torch.ones(6, dtype=torch.bool)):
        with pytest.raises(RuntimeError, match='mask'):
            v.update(bad)
    with pytest.raises(RuntimeError, match='GPU'):
        v.update()
    bare = cuda.ViewFields(grid, scenery, points, 10., None, 0., grid.free, None, None, None, new((2, 3), torch.int32), None)
    with pytest.raises(RuntimeError, match='store=False'):
        bare.image(0)
    # a ViewFields is a layer as it is: its bytes, a store a viewpoint
    layer = cuda.cell_layer(v)
    assert layer.values is v.values and layer.n_fields == 3 and not layer.is_float
    assert cuda.map_channel(v, where=False).source.values is v.values
    with pytest.raises(RuntimeError):
        cuda.cell_layer(bare)


def test_best_views_choose_on_hand_filled_tensors():
    from megastep_amd import modules
    inf = float('inf')
    gains = torch.tensor([[[4, 8, 8, 0], [6, 6, 6, 6]], [[0, 0, 0, 0], [5, 9, 1, 1]], [[3, 3, 3, 3], [7, 2, 2, 7]]], dtype=torch.int32)
    distances = torch.tensor([[[1., 3., 3., .1], [2., 2., inf, 1.]], [[1., 1., 1., 1.], [inf, inf, inf, inf]],
                              [[inf, 0., 0., inf], [float('nan'), 1., 1., 3.]]])
    index, none = modules.BestViews.choose(gains, distances)
    assert index.dtype == torch.int64 and none.dtype == torch.bool and index.shape == none.shape == (3, 2)
    # 4/2 = 8/4 = 8/4: a tie of three, the first; 6/2 < 6/3 ... the nearest of equal gains, not the one no path reaches
    # (7/4 beats 2/2; the NaN distance's 7 is not in the running)
    assert index.tolist() == [[0, 3], [0, 0], [1, 3]]
    # all gains zero -> none; all distances infinite -> none; a NaN distance is not finite
    assert none.tolist() == [[False, False], [True, True], [False, False]]
    index, none = modules.BestViews.choose(gains, distances, d0=0.)
    assert index.tolist() == [[0, 3], [0, 0], [1, 3]] and none.tolist() == [[False, False], [True, True], [False, False]]
    # the rule restated: the first index of the largest score among the valid ones
    rng = np.random.RandomState(2)
    g = torch.as_tensor(rng.randint(0, 4, (50, 3, 8)).astype(np.int32))
    d = torch.as_tensor(np.where(rng.rand(50, 3, 8) < .2, np.inf, rng.randint(0, 3, (50, 3, 8))).astype(F))
    index, none = modules.BestViews.choose(g, d)
    for n in range(50):
        for a in range(3):
            scores = [float(g[n, a, k])/(float(d[n, a, k]) + 1.) if np.isfinite(float(d[n, a, k])) and g[n, a, k] > 0 else None for k in range(8)]
            valid = [s for s in scores if s is not None]
            assert bool(none[n, a]) == (not valid)
            assert int(index[n, a]) == (scores.index(max(valid)) if valid else 0)
    with pytest.raises(RuntimeError, match="kind must be"):
        from megastep_amd.demo.envs.floorcoverage import FloorCoverage
        FloorCoverage.expert(None, kind='nearest')
