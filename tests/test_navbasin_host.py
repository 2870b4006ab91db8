"""Basins (include/megastep_hip.h, MsNavBasins / MsNavBasinQuery / MsNavPointMarks) restated in numpy and plain
Python - basin_rule, point_mark_rule and basin_query_rule, which follow chains cell by cell with a scalar restatement of the hop
rule, written apart from the kernel's text - and the host instantiations of the kernels' own per-cell functions
(ms_host_nav_basins, ms_host_nav_basin_query, ms_host_nav_point_marks: csrc/kernels/navbasin.h) held to EQUALITY with them. No
GPU: what is compared is the text every lane of the kernels evaluates, swept serially."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from tests.test_abi import ROOT, declared_symbols
from tests.test_navfield_host import CELL, CELLS, RADIUS, F, INF, nav_rule
from tests.test_navpath_host import NEIGHBOURS, path_rule
from tests.test_navseed_host import host_follow, seed_rule
from tests.test_navregion_host import _Host, _max_framed, serpentine

DIAGONAL = F(1.41421356)
INT_MAX = 2**31 - 1


class basin_rule:
    """The contract in numpy and plain Python: one cell, one hop, one chain at a time."""

    @staticmethod
    def hop(free, D, cell, i, j):
        """The hop from cell (i, j) of a seeded field: (0, i, j) the chain ends here, (1, i', j') on to that cell, (-1, i, j)
        broken. Scalars throughout: every sum is one binary32 addition."""
        ny, nx = D.shape
        here = D[i, j]
        if here == 0:                                                    # (-0.f too)
            return 0, i, j
        is_free = lambda a, b: 0 <= a < ny and 0 <= b < nx and bool(free[a, b])
        best, below, found = INF, INF, None
        for t, (di, dj) in enumerate(NEIGHBOURS):
            ui, uj = i + di, j + dj
            if not is_free(ui, uj) or (t >= 4 and not (is_free(ui, j) and is_free(i, uj))):
                continue
            du = D[ui, uj]
            v = du + (F(cell)*DIAGONAL if t >= 4 else F(cell))
            if v < best:
                best, below, found = v, du, (ui, uj)
        if found is None or not (below < here):
            return -1, i, j
        return 1, found[0], found[1]

    @staticmethod
    def succ(free, D, cell):
        """(ny*nx,) int64: every cell's successor - itself on a seed, -1 where the cell is blocked, its value is not < +inf or no
        hop leads on - by the scalar hop."""
        ny, nx = D.shape
        out = np.full(ny*nx, -1, np.int64)
        with np.errstate(all='ignore'):
            for k in np.flatnonzero(free.reshape(-1) & (D.reshape(-1) < INF)):
                kind, i, j = basin_rule.hop(free, D, cell, int(k)//nx, int(k) % nx)
                if kind >= 0:
                    out[k] = i*nx + j
        return out

    @staticmethod
    def succ_by_table(free, D, cell, geom=(0, 0, 0, 0)):
        """The same from seed_rule.hops, every cell's hop at once (tests/test_navseed_host.py): for grids too large for the scalar
        hop. test_the_two_statements_of_the_successor_agree holds the two together."""
        ny, nx = D.shape
        kind, step, _ = seed_rule.hops((geom, cell, free, D))
        di, dj = np.array(NEIGHBOURS)[np.maximum(step, 0)].reshape(ny, nx, 2).transpose(2, 0, 1)
        i, j = np.indices((ny, nx))
        target = np.where(kind == 1, (i + di)*nx + (j + dj), np.where(kind == 0, i*nx + j, -1))
        with np.errstate(all='ignore'):
            return np.where(free & (D < INF), target, -1).reshape(-1).astype(np.int64)

    @staticmethod
    def ends(succ):
        """(end, hops): the cell each cell's chain ends on (-1: none - dead, or its chain breaks) and the hops there, chain by
        chain, cell by cell; a chain that runs into one already followed takes over what that one found."""
        succ = np.asarray(succ).tolist()                                 # (plain lists: a large grid is a long loop)
        n = len(succ)
        end, hops = [-2]*n, [0]*n
        for k in range(n):
            trail, v = [], k
            while end[v] == -2:
                s = succ[v]
                if s == v or s < 0:
                    end[v] = s
                    break
                trail.append(v)
                assert len(trail) <= n                                   # (D falls at every hop: no cycle)
                v = s
            e, length = end[v], hops[v]
            for u in reversed(trail):
                length += 1
                end[u], hops[u] = e, length
        end, hops = np.array(end, np.int64).reshape(-1), np.array(hops, np.int64).reshape(-1)
        return end, hops

    @staticmethod
    def call(geom, starts, cell, free, values, G=1, ids=None, n_ids=0, mask=None, before=None, table=False):
        """One call of ms_nav_basins: dict of labels (flat, the fields' layout), sizes (N, G, K), reached (N, G) and `longest`
        (N, G): the longest chain in hops (not an output: the bound on passes). `before`: what the outputs held."""
        N = len(geom)
        size = max(G*int(starts[-1]), 1)
        out = before if before is not None else dict(labels=np.full(size, -1, np.int32), sizes=np.zeros((N, G, n_ids), np.int32),
                                                     reached=np.zeros((N, G), np.int32))
        out = {k: np.array(v) for k, v in out.items()}
        out['longest'] = np.zeros((N, G), np.int64)
        for n in range(N):
            jx0, iy0, nx, ny = (int(v) for v in geom[n])
            cells = nx*ny if nx > 0 and ny > 0 else 0
            for g in range(G):
                if mask is not None and not mask[n][g]:
                    continue
                out['sizes'][n, g], out['reached'][n, g] = 0, 0
                if cells == 0:
                    continue
                at = G*int(starts[n]) + g*cells
                fr = (np.asarray(free)[int(starts[n]):int(starts[n]) + cells].reshape(ny, nx) & 1) != 0
                D = np.asarray(values, F)[at:at + cells].reshape(ny, nx)
                succ = basin_rule.succ_by_table(fr, D, cell, (jx0, iy0, nx, ny)) if table else basin_rule.succ(fr, D, cell)
                end, hops = basin_rule.ends(succ)
                labels = end if ids is None else np.where(end >= 0, np.asarray(ids)[at:at + cells][np.maximum(end, 0)], -1)
                labels = np.where(end >= 0, labels, -1).astype(np.int32)
                out['labels'][at:at + cells] = labels
                out['reached'][n, g] = (labels >= 0).sum()
                counted = labels[(labels >= 0) & (labels < n_ids)]
                out['sizes'][n, g] = np.bincount(counted, minlength=n_ids)[:n_ids] if n_ids else 0
                out['longest'][n, g] = hops.max(initial=0)
        return out


def _field_of(G, field, n, p):
    f = int(field[n][p]) if field is not None else (0 if G == 1 else p)
    return f if 0 <= f < G else -1


class point_mark_rule:
    @staticmethod
    def call(geom, starts, cell, free, points, G=1, point_ids=None, field=None):
        """(marks uint8, ids int32), flat in the fields' layout: every free anchor cell of every point."""
        size = max(G*int(starts[-1]), 1)
        marks, ids = np.zeros(size, np.uint8), np.full(size, INT_MAX, np.int32)
        N, P = points.shape[:2]
        for n in range(N):
            jx0, iy0, nx, ny = (int(v) for v in geom[n])
            if nx <= 0 or ny <= 0:
                continue
            fr = (np.asarray(free)[int(starts[n]):int(starts[n]) + nx*ny].reshape(ny, nx) & 1) != 0
            for p in range(P):
                f = _field_of(G, field, n, p)
                corner = path_rule.corner(points[n, p], (jx0, iy0, nx, ny), cell)
                if f < 0 or corner is None:
                    continue
                at = G*int(starts[n]) + f*nx*ny
                for t in range(4):
                    i, j = corner[0] + (t >> 1), corner[1] + (t & 1)
                    if 0 <= i < ny and 0 <= j < nx and fr[i, j]:
                        marks[at + i*nx + j] = 1
                        ids[at + i*nx + j] = min(int(ids[at + i*nx + j]), int(point_ids[n][p]) if point_ids is not None else p)
        return marks, ids


class basin_query_rule:
    @staticmethod
    def call(geom, starts, cell, free, values, labels, G, points, field=None):
        """(N, P) int32: the label at the anchor path_rule.start picks; -1 without one."""
        N, P = points.shape[:2]
        out = np.full((N, P), -1, np.int32)
        for n in range(N):
            jx0, iy0, nx, ny = (int(v) for v in geom[n])
            if nx <= 0 or ny <= 0:
                continue
            fr = (np.asarray(free)[int(starts[n]):int(starts[n]) + nx*ny].reshape(ny, nx) & 1) != 0
            for p in range(P):
                f = _field_of(G, field, n, p)
                if f < 0:
                    continue
                at = G*int(starts[n]) + f*nx*ny
                D = np.asarray(values, F)[at:at + nx*ny].reshape(ny, nx)
                with np.errstate(all='ignore'):
                    first = path_rule.start(((jx0, iy0, nx, ny), cell, fr, D, None), points[n, p])
                if first is not None:
                    out[n, p] = labels[at + first[0]*nx + first[1]]
        return out


# ---------------------------------------------------------------------------------------------------------------------
# the host instantiations
# ---------------------------------------------------------------------------------------------------------------------
class _BasinHost(_Host):
    """The three host entries on one grid of host arrays; the outputs start as sentinels."""

    def basins(self, values, G=1, ids=None, n_ids=0, mask=None, before=None, passes=True):
        from megastep_amd import _lib
        size = max(G*int(self.starts[-1]), 1)
        out = before if before is not None else dict(labels=np.full(size, -7, np.int32), sizes=np.full((self.N, G, n_ids), -7, np.int32),
                                                     reached=np.full((self.N, G), -7, np.int32))
        out = {k: np.ascontiguousarray(v).copy() for k, v in out.items()}
        out['passes'] = np.full((self.N, G), -7, np.int32) if passes else None
        values = np.ascontiguousarray(np.concatenate([np.asarray(values, F).reshape(-1), np.zeros(1, F)]))
        ids = None if ids is None else np.ascontiguousarray(np.concatenate([np.asarray(ids, np.int32).reshape(-1), np.zeros(1, np.int32)]))
        mask = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        ptr = lambda a: None if a is None else a.ctypes.data
        spec = _lib.MsNavBasins(G, values.ctypes.data, ptr(ids), n_ids, ptr(mask), out['labels'].ctypes.data,
                                out['sizes'].ctypes.data if n_ids else None, out['reached'].ctypes.data, ptr(out['passes']))
        assert self.h.ms_host_nav_basins(ctypes.byref(self.grid), ctypes.byref(spec)) == 0
        return out

    def at(self, values, labels, G, points, field=None):
        from megastep_amd import _lib
        points = np.ascontiguousarray(points, F)
        N, P = points.shape[:2]
        values = np.ascontiguousarray(np.concatenate([np.asarray(values, F).reshape(-1), np.zeros(1, F)]))
        labels = np.ascontiguousarray(labels, np.int32)
        field = None if field is None else np.ascontiguousarray(field, np.int32)
        out = np.full((N, P), -7, np.int32)
        spec = _lib.MsNavBasinQuery(P, points.ctypes.data, None if field is None else field.ctypes.data, values.ctypes.data,
                                    labels.ctypes.data, G, out.ctypes.data)
        assert self.h.ms_host_nav_basin_query(ctypes.byref(self.grid), ctypes.byref(spec)) == 0
        return out

    def marks(self, points, G=1, point_ids=None, field=None):
        from megastep_amd import _lib
        points = np.ascontiguousarray(points, F)
        P = points.shape[1]
        size = max(G*int(self.starts[-1]), 1)
        marks, ids = np.zeros(size, np.uint8), np.full(size, INT_MAX, np.int32)
        point_ids = None if point_ids is None else np.ascontiguousarray(point_ids, np.int32)
        field = None if field is None else np.ascontiguousarray(field, np.int32)
        ptr = lambda a: None if a is None else a.ctypes.data
        spec = _lib.MsNavPointMarks(P, points.ctypes.data, ptr(field), ptr(point_ids), G, marks.ctypes.data, ids.ctypes.data)
        assert self.h.ms_host_nav_point_marks(ctypes.byref(self.grid), ctypes.byref(spec)) == 0
        return marks, ids


KEYS = ('labels', 'sizes', 'reached')


def same(got, want):
    for key in KEYS:
        assert np.array_equal(got[key], want[key]), (key, int((np.asarray(got[key]) != np.asarray(want[key])).sum()))


def bound(longest):
    """The most passes a field whose longest chain has `longest` hops may take: a slot is min(2^t, length) hops ahead after t
    passes, then the pass that sees no change, and one of slack."""
    return math.ceil(math.log2(max(int(longest), 1))) + 2


class _World:
    """Envs laid out by hand: [(geom, free (ny, nx) bool, [seeds (ny, nx) bool]*G)], the fields by seed_rule's Dijkstra."""

    def __init__(self, envs, G=1, cell=CELL, clearance=RADIUS):
        self.cell, self.clearance = cell, clearance
        self.geom = np.array([g for g, _, _ in envs], np.int32)
        self.images = [np.asarray(f, bool) for _, f, _ in envs]
        self.starts = np.concatenate([[0], np.cumsum([f.size for f in self.images])]).astype(np.int64)
        self.free = np.concatenate([f.reshape(-1) for f in self.images] + [np.zeros(0, bool)]).astype(np.uint8)
        self.G, self.N = G, len(envs)
        self.seeds = [[np.asarray(s, bool) & f for s in seeds] for (_, _, seeds), f in zip(envs, self.images)]
        self.values = np.concatenate([seed_rule.field(f, cell, s).reshape(-1) if f.size else np.zeros(0, F)
                                      for f, seeds in zip(self.images, self.seeds) for s in seeds] + [np.zeros(0, F)]).astype(F)

    def host(self, **kw):
        return _BasinHost(self.geom, self.starts, self.free, cell=self.cell, clearance=self.clearance, **kw)

    def rule(self, values=None, **kw):
        return basin_rule.call(self.geom, self.starts, self.cell, self.free, self.values if values is None else values, self.G, **kw)

    def at(self, n, g=0):
        cells = self.images[n].size
        return self.G*int(self.starts[n]) + g*cells, cells

    def centre(self, n, i, j, di=0., dj=0.):
        return [(int(self.geom[n][0]) + j + .5 + dj)*self.cell, (int(self.geom[n][1]) + i + .5 + di)*self.cell]


def _cells(shape, *cells):
    m = np.zeros(shape, bool)
    for i, j in cells:
        m[i, j] = True
    return m


def junction():
    """(7, 9): a corridor along row 3 with a seed at each end, and a stem up column 4 from its middle: the stem and the junction
    are as far from the one seed as from the other."""
    m = np.zeros((7, 9), bool)
    m[3, :] = True
    m[3:, 4] = True
    return m


_HAND = []


def hand():
    """Seven envs by hand, one field each; env 4 has no cells, env 5 no seed, env 6 more cells than the smallest launch holds."""
    if not _HAND:
        rng = np.random.RandomState(5)
        room = np.ones((9, 12), bool)
        room[4, 2:9] = False
        blobs = rng.rand(17, 23) < .8
        strip = np.ones((3, 3400), bool)
        strip[1, 5:3395] = rng.rand(3390) < .7
        _HAND.append(_World([((0, 0, 12, 9), room, [_cells((9, 12), (1, 1))]),                       # 0: one seed
                             ((-3, 2, 12, 9), room, [_cells((9, 12), (6, 5), (6, 6), (0, 11))]),     # 1: two adjacent seeds and a third
                             ((5, -4, 9, 7), junction(), [_cells((7, 9), (3, 0), (3, 8))]),          # 2: ties at the junction
                             ((-8, -8, 23, 17), blobs, [rng.rand(17, 23) < .03]),                    # 3: random, several seeds
                             ((2, 2, 0, 5), np.zeros((5, 0), bool), [np.zeros((5, 0), bool)]),       # 4: no cells
                             ((0, 0, 6, 5), np.ones((5, 6), bool), [np.zeros((5, 6), bool)]),        # 5: no seed
                             ((-2000, 0, 3400, 3), strip, [_cells((3, 3400), (1, 0), (1, 3399), (0, 1700))])]))      # 6: 10 200 cells
    return _HAND[0]


def _index(point, geom, cell=CELL):
    jx0, iy0, nx, ny = geom
    j, i = int(np.floor(float(point[0])/cell)) - jx0, int(np.floor(float(point[1])/cell)) - iy0
    assert 0 <= i < ny and 0 <= j < nx
    return i*nx + j


@pytest.mark.parametrize('launch', ['fits', 'stored'])
def test_on_the_hand_made_grids_the_label_is_the_cell_the_path_ends_on(launch):
    """At a cell of 0.125 only: that most paths start on the very cell they are asked from (`own > .8*checked`) is a property of
    centres that are exact in binary32, not of the kernel."""
    w = hand()
    from megastep_amd import nav
    assert nav.BASIN_CAPACITY[0] < w.images[6].size <= _max_framed(w.geom) <= nav.BASIN_CAPACITY[1]
    got = (w.host() if launch == 'fits' else _stored(w)).basins(w.values)      # (stored: env 6 is jumped in its labels store)
    want = w.rule()
    same(got, want)
    assert all(1 <= got['passes'][n, 0] <= bound(want['longest'][n, 0]) for n in (0, 1, 2, 3, 6)) and want['longest'][6, 0] > 800
    assert (got['passes'][[0, 1, 2, 3], 0] >= 1).all() and got['passes'][4, 0] == 0 and got['reached'][4, 0] == 0
    # a field without seeds: all -1
    at, cells = w.at(5)
    assert (got['labels'][at:at + cells] == -1).all() and got['reached'][5, 0] == 0 and got['passes'][5, 0] == 1
    # the seeds name themselves; the one-seed env is all one label
    at, cells = w.at(0)
    assert set(got['labels'][at:at + cells].tolist()) == {-1, 1*12 + 1} and got['reached'][0, 0] == int(w.images[0].sum())
    at, cells = w.at(1)
    assert got['labels'][at + 6*12 + 5] == 6*12 + 5 and got['labels'][at + 6*12 + 6] == 6*12 + 6 and got['labels'][at + 11] == 11
    assert set(got['labels'][at:at + cells].tolist()) == {-1, 11, 6*12 + 5, 6*12 + 6}
    # the junction's ties: both labels occur, and every cell of the stem has the one the path from it ends on
    at, cells = w.at(2)
    assert set(got['labels'][at:at + cells].tolist()) == {-1, 3*9, 3*9 + 8}
    stem = got['labels'][at:at + cells].reshape(7, 9)[3:, 4]
    assert len(set(stem.tolist())) == 1 and stem[0] >= 0
    checked = own = 0
    host = w.host()
    for n in range(4):
        at, cells = w.at(n)
        D = w.values[at:at + cells].reshape(w.images[n].shape)
        geom = tuple(int(v) for v in w.geom[n])
        open_cells = np.flatnonzero(w.images[n].reshape(-1))
        centres = np.array([w.centre(n, k//geom[2], k % geom[2]) for k in open_cells], F)
        points = np.full((w.N, len(open_cells), 2), np.nan, F)
        points[n] = centres
        asked = host.at(w.values, got['labels'], 1, points)
        assert (asked[np.arange(w.N) != n] == -1).all()
        for k, p, answer in zip(open_cells, centres, asked[n]):
            pts, count = host_follow((geom, CELL, w.images[n], D), p, max_points=cells + 2)
            if np.isfinite(D.reshape(-1)[k]):
                # the path starts at the anchor the query's minimum is attained at - the cell itself, or a neighbour a rounding nearer
                first, last = _index(pts[1], geom), _index(pts[count - 1], geom)
                assert count >= 2 and got['labels'][at + first] == last == answer, (n, k)
                checked += 1
                own += first == k
            else:
                assert count == 0 and got['labels'][at + k] == -1 and answer == -1
    assert checked > 300 and own > .8*checked


def _stored(w):
    """A host whose launch is the smallest, and whose envs of more cells than its capacity run in the labels store."""
    return w.host(max_framed=0)


def test_an_env_too_large_for_the_launch_is_jumped_in_its_labels_store_to_the_same_result():
    from megastep_amd import _lib, nav
    caps = (ctypes.c_int*3)()
    assert _lib.lib().ms_host_nav_basin_capacity(caps) == 0 and tuple(caps) == nav.BASIN_CAPACITY
    assert tuple(caps) == tuple((kib*1024 - 64)//4 - 256 for kib in (40, 80, 160))
    rng = np.random.RandomState(9)
    free = rng.rand(101, 103) < .75
    w = _World([((-50, 7, 103, 101), free, [rng.rand(101, 103) < .002, _cells((101, 103), *np.argwhere(free)[:1])]),
                ((0, 0, 7, 5), np.ones((5, 7), bool), [_cells((5, 7), (0, 0)), _cells((5, 7), (4, 6), (0, 6))])], G=2)
    assert w.images[0].size > caps[0] and _max_framed(w.geom) <= caps[1]
    ids = rng.randint(-2, 6, 2*int(w.starts[-1])).astype(np.int32)
    want = w.rule(ids=ids, n_ids=4)
    framed, stored = w.host().basins(w.values, 2, ids, 4), _stored(w).basins(w.values, 2, ids, 4)
    same(framed, want)
    same(stored, want)
    assert (want['reached'][0] > 1000).all() and (want['sizes'][0].sum(-1) < want['reached'][0]).all()
    print('passes, in a copy and as stored:', framed['passes'].reshape(-1).tolist(), stored['passes'].reshape(-1).tolist())
    for got in (framed, stored):
        assert all(1 <= got['passes'][n, g] <= bound(want['longest'][n, g]) for n in range(2) for g in range(2))


@pytest.mark.parametrize('which', [0, 1, 2])
def test_every_capacity_at_the_side_that_just_fits_and_the_next_one(which):
    """A serpentine corridor from a seed at its start is one chain of about side*side/2 hops: the doubling bound on the passes is
    a condition."""
    from megastep_amd import nav
    capacity = nav.BASIN_CAPACITY[which]
    s = math.isqrt(capacity)
    assert s*s <= capacity < (s + 1)*(s + 1)
    for side in (s, s + 1):
        w = _World([((-3, 5, side, side), serpentine(side), [_cells((side, side), (0, 0))])])
        want = w.rule()
        got = w.host(max_framed=capacity).basins(w.values)               # (this capacity's launch: side s in a copy, s + 1 as stored)
        same(got, want)
        corridor = int(serpentine(side).sum())
        assert want['reached'][0, 0] == corridor and want['longest'][0, 0] == corridor - 1
        assert set(got['labels'].tolist()) == {-1, 0}
        print('capacity', capacity, 'side', side, 'longest chain', int(want['longest'][0, 0]), 'passes', int(got['passes'][0, 0]))
        assert 1 <= got['passes'][0, 0] <= bound(want['longest'][0, 0])


def test_mask_leaves_unmarked_fields_as_out_held_them():
    w = hand()
    two = _World([(tuple(g), f, [s[0], np.roll(s[0], 3)]) for g, f, s in zip(w.geom, w.images, w.seeds)], G=2)
    mask = np.ones((two.N, 2), np.uint8)
    mask[1, 0] = mask[3, 1] = mask[4, 0] = 0
    rng = np.random.RandomState(2)
    ids = rng.randint(0, 3, 2*int(two.starts[-1]) + 1).astype(np.int32)
    got = two.host().basins(two.values, 2, ids[:-1], 3, mask)
    before = dict(labels=np.full_like(got['labels'], -7), sizes=np.full_like(got['sizes'], -7), reached=np.full_like(got['reached'], -7))
    same(got, two.rule(ids=ids[:-1], n_ids=3, mask=mask, before=before))
    at, cells = two.at(1, 0)
    assert (got['labels'][at:at + cells] == -7).all() and (got['sizes'][1, 0] == -7).all() and got['reached'][3, 1] == -7 and got['passes'][1, 0] == -7
    assert (got['sizes'][4, 1] == 0).all() and got['reached'][4, 1] == 0 and got['reached'][4, 0] == -7
    assert (got['sizes'][mask != 0].sum(-1) == got['reached'][mask != 0]).all()


@pytest.mark.parametrize('kind', ['pit', 'nan', '-inf', '-0'])
def test_stale_fields_break_chains_and_the_call_returns(kind):
    w = hand()
    values = w.values.copy()
    broken = 0
    for n in (0, 1, 3):
        at, cells = w.at(n)
        D = values[at:at + cells]
        finite = np.flatnonzero(np.isfinite(D) & (D > F(3*CELL)))
        seeds = np.flatnonzero(D == 0)
        rng = np.random.RandomState(n)
        if kind == 'pit':
            D[rng.choice(finite, 2)] = F(1e-3)                           # (not a seed, and lower than every neighbour)
        elif kind == 'nan':
            D[rng.choice(finite, 2)] = F(np.nan)
        elif kind == '-inf':
            D[rng.choice(finite, 2)] = F(-np.inf)
        else:
            D[seeds[:1]] = F(-0.)
    want = w.rule(values)
    for host in (w.host(), _stored(w)):
        got = host.basins(values)
        same(got, want)
    clean = w.rule()
    for n in (0, 1, 3):
        at, cells = w.at(n)
        broken += int(((want['labels'][at:at + cells] == -1) & (clean['labels'][at:at + cells] >= 0)).sum())
    if kind == '-0':
        assert broken == 0 and np.array_equal(want['labels'], clean['labels'])      # (a -0.f seed is a seed)
    elif kind == 'nan':
        assert broken >= 3                                               # (the cells themselves, at the least)
    else:
        assert broken > 6                                                # (more than the edited cells: whatever drains into them)


@pytest.mark.parametrize('n_ids', [1, 2, 256])
def test_ids_and_sizes(n_ids):
    w = hand()
    rng = np.random.RandomState(n_ids)
    total = int(w.starts[-1])
    host = w.host()
    # every id in range: the sizes add up to the reached cells
    ids = rng.randint(0, n_ids, total).astype(np.int32)
    got = host.basins(w.values, 1, ids, n_ids)
    same(got, w.rule(ids=ids, n_ids=n_ids))
    assert np.array_equal(got['sizes'].sum(-1), got['reached']) and got['reached'].sum() > 300
    # ids beyond n_ids and negative ids: counted nowhere, and a negative one is no basin
    ids = rng.randint(-3, n_ids + 40, total).astype(np.int32)
    for n in range(4):
        at, cells = w.at(n)
        seeds = np.flatnonzero(w.values[at:at + cells] == 0)
        ids[at + seeds] = rng.choice([-2, 0, n_ids - 1, n_ids, n_ids + 7], len(seeds))
    ids[w.at(1)[0] + np.array([6*12 + 5, 6*12 + 6, 11])] = [-2, n_ids, 0]  # (every kind for sure)
    got = host.basins(w.values, 1, ids, n_ids)
    want = w.rule(ids=ids, n_ids=n_ids)
    same(got, want)
    assert (got['sizes'].sum(-1) <= got['reached']).all() and (got['sizes'].sum(-1) < got['reached']).any()
    plain = w.rule()
    assert (got['reached'] <= plain['reached']).all() and got['reached'][1, 0] < plain['reached'][1, 0]
    # without ids and with sizes: the labels are cell indices, counted where they are below n_ids
    got = host.basins(w.values, 1, None, n_ids)
    same(got, w.rule(n_ids=n_ids))


def test_the_two_statements_of_the_successor_agree():
    w = hand()
    values = w.values.copy()
    at, cells = w.at(3)
    edit = at + np.flatnonzero(np.isfinite(values[at:at + cells]))[::9]
    values[edit] = np.resize(np.array([np.nan, -np.inf, .01, np.inf], F), len(edit))
    same(w.rule(values), w.rule(values, table=True))


# ---------------------------------------------------------------------------------------------------------------------
# the six plans: seeds by point marks at two points an env, queries from every spawn point
# ---------------------------------------------------------------------------------------------------------------------
_PLANS = {}


def plan_world(cell=CELL, r=RADIUS):
    """(w, marks, ids, points): test_navseed_host's six plans as one grid of one field an env, seeded by point_mark_rule at two
    spawn points an env."""
    if (cell, r) not in _PLANS:
        from tests.test_navseed_host import cases
        cs = cases(cell, r)[::2]
        rng = np.random.RandomState(23)
        geom = np.array([c.geom for c in cs], np.int32)
        starts = np.concatenate([[0], np.cumsum([c.free.size for c in cs])]).astype(np.int64)
        free = np.concatenate([c.free.reshape(-1) for c in cs]).astype(np.uint8)
        points = np.stack([(c.points[rng.choice(len(c.points), 2, replace=False)] + rng.uniform(-.05, .05, (2, 2))).astype(F) for c in cs])
        marks, ids = point_mark_rule.call(geom, starts, cell, free, points)
        w = _World([(tuple(c.geom), c.free, [marks[starts[n]:starts[n + 1]].reshape(c.free.shape) != 0]) for n, c in enumerate(cs)],
                   cell=cell, clearance=r)
        w.cases = cs
        _PLANS[cell, r] = (w, marks, ids, points)
    return _PLANS[cell, r]


def test_on_the_six_plans_point_marks_and_basins_are_the_rules():
    _point_marks_and_basins_are_the_rules(*plan_world())


@pytest.mark.parametrize('cell,r', CELLS)
def test_point_marks_and_basins_are_the_rules_at_other_cell_widths(cell, r):
    _point_marks_and_basins_are_the_rules(*plan_world(cell, r))


def _point_marks_and_basins_are_the_rules(w, marks, ids, points):
    host = w.host()
    got_marks, got_ids = host.marks(points)
    assert np.array_equal(got_marks, marks) and np.array_equal(got_ids, ids)
    assert all(1 <= marks[w.starts[n]:w.starts[n + 1]].sum() <= 8 for n in range(6)) and set(ids[marks != 0].tolist()) == {0, 1}
    got = host.basins(w.values, 1, ids, 2)
    want = w.rule(ids=ids, n_ids=2)
    same(got, want)
    assert np.array_equal(got['sizes'].sum(-1), got['reached']) and (got['sizes'] > 100*(CELL/w.cell)**2).all()      # (the same floor, in cells)
    print('passes of the serial sweeps on the six plans:', got['passes'].reshape(-1).tolist(), 'longest chains:', want['longest'].reshape(-1).tolist())
    assert all(1 <= got['passes'][n, 0] <= bound(want['longest'][n, 0]) for n in range(6))


def test_on_the_six_plans_the_query_from_every_spawn_point_is_the_cell_its_path_ends_on():
    assert _query_is_the_cell_the_path_ends_on(*plan_world()) > 15000


@pytest.mark.parametrize('cell,r', CELLS)
def test_the_query_is_the_cell_the_path_ends_on_at_other_cell_widths(cell, r):
    """From every fourth spawn point of the same plans; the spawn points themselves do not move with the cell."""
    assert _query_is_the_cell_the_path_ends_on(*plan_world(cell, r), stride=4) > 15000/4*.9


def _query_is_the_cell_the_path_ends_on(w, marks, ids, points, stride=1):
    host = w.host()
    cells_of = host.basins(w.values)['labels']                           # (no ids: a label is the seed's cell)
    owners = host.basins(w.values, 1, ids, 2)['labels']
    asked = [c.points[::stride] for c in w.cases]
    P = max(len(a) for a in asked)
    spawns = np.full((6, P, 2), np.nan, F)
    for n, a in enumerate(asked):
        spawns[n, :len(a)] = a
    field = np.zeros((6, P), np.int32)
    got = host.at(w.values, cells_of, 1, spawns, field)
    assert np.array_equal(got, basin_query_rule.call(w.geom, w.starts, w.cell, w.free, w.values, cells_of, 1, spawns, field))
    assert np.array_equal(got, host.at(w.values, cells_of, 1, spawns))    # (one field: the default asks it)
    who = host.at(w.values, owners, 1, spawns)
    found = 0
    for n, c in enumerate(w.cases):
        at, cells = w.at(n)
        assert (got[n, len(asked[n]):] == -1).all()                      # (the NaN points)
        for k, p in enumerate(asked[n]):
            pts, count = host_follow(c.world[:3] + (w.values[at:at + cells].reshape(c.free.shape),), p, max_points=cells + 2)
            if count == 0:
                assert got[n, k] == -1 and who[n, k] == -1
                continue
            assert count >= 2                                            # (a converged field: no chain breaks)
            cell = _index(pts[count - 1], tuple(c.geom), w.cell)
            assert got[n, k] == cell and who[n, k] == ids[at + cell], (n, k)
            found += 1
    assert set(np.unique(who).tolist()) >= {0, 1}
    return found


# ---------------------------------------------------------------------------------------------------------------------
# point marks
# ---------------------------------------------------------------------------------------------------------------------
def test_point_marks_shared_anchors_walls_nans_and_bad_fields():
    w = hand()
    host = w.host()
    points = np.full((w.N, 5, 2), np.nan, F)
    for n in (0, 1, 2, 3, 5):
        points[n, 0] = w.centre(n, 2, 2, .5, .5)                         # (a corner: four anchors)
        points[n, 1] = w.centre(n, 2, 3, .5, .5)                         # (the next corner: shares two of them)
        points[n, 3] = [F(2.**31), 0.]
    points[2, 0], points[2, 1] = w.centre(2, 0, 0, .5, .5), w.centre(2, 3, 3, .2, -.2)      # (all anchors blocked; two of four free)
    points[0, 4] = w.centre(0, 8, 11, .5, .5)                            # (one anchor in the grid)
    for G, field, point_ids in ((1, None, None), (1, None, np.tile(np.array([9, 4, 1, 0, 7], np.int32), (w.N, 1))),
                                (5, None, None), (3, np.tile(np.array([2, 2, 0, -1, 3], np.int32), (w.N, 1)), None)):
        got = host.marks(points, G, point_ids, field)
        want = point_mark_rule.call(w.geom, w.starts, CELL, w.free, points, G, point_ids, field)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (G,)
        assert np.array_equal(got[1] != INT_MAX, got[0] != 0)
    marks, ids = host.marks(points)
    at = int(w.starts[0])
    assert ids[at + 2*12 + 3] == 0 and ids[at + 3*12 + 3] == 0 and ids[at + 2*12 + 4] == 1 and ids[at + 2*12 + 2] == 0      # (the lower id stays)
    assert marks[at:at + 108].sum() == 7 and marks[at + 8*12 + 11] == 1
    at = int(w.starts[2])
    assert marks[at:at + 63].tolist() == _cells((7, 9), (3, 2), (3, 3)).reshape(-1).astype(int).tolist()
    marks, ids = host.marks(points, 1, np.tile(np.array([9, 4, 1, 0, 7], np.int32), (w.N, 1)))
    at = int(w.starts[0])
    assert ids[at + 2*12 + 3] == 4 and ids[at + 2*12 + 2] == 9 and ids[at + 2*12 + 4] == 4
    marks, ids = host.marks(points, 3, None, np.tile(np.array([2, 2, 0, -1, 3], np.int32), (w.N, 1)))
    assert not marks[3*int(w.starts[0]):][:108].any() and marks[3*int(w.starts[0]) + 2*108:][:108].sum() == 6      # (point 4's field 3 is no field)


# ---------------------------------------------------------------------------------------------------------------------
# header, loader, refusals
# ---------------------------------------------------------------------------------------------------------------------
ENTRIES = {'ms_nav_basins', 'ms_nav_basin_query', 'ms_nav_point_marks'}
HOOKS = {'ms_host_nav_basins', 'ms_host_nav_basin_query', 'ms_host_nav_point_marks', 'ms_host_nav_basin_capacity'}


def test_the_header_declares_the_calls_and_the_loader_binds_them():
    from megastep_amd import _lib
    assert ENTRIES <= set(declared_symbols(('megastep_hip.h',))) and HOOKS <= set(declared_symbols(('megastep_hip_test.h',)))
    assert ENTRIES | HOOKS <= set(_lib.SYMBOLS)
    text = open(os.path.join(ROOT, 'include', 'megastep_hip.h')).read()
    assert int(re.search(r'#define MS_ABI_VERSION (\d+)', text).group(1)) == _lib.ABI_VERSION
    handle = _lib.lib()
    assert all(hasattr(handle, name) for name in ENTRIES | HOOKS)


@pytest.mark.parametrize('name, fields', [
    ('MsNavBasins', ('n_fields', 'fields', 'ids', 'n_ids', 'mask', 'labels', 'sizes', 'reached', 'passes')),
    ('MsNavBasinQuery', ('n_points', 'points', 'field', 'fields', 'labels', 'n_fields', 'out')),
    ('MsNavPointMarks', ('n_points', 'points', 'field', 'point_ids', 'n_fields', 'marks', 'ids'))])
def test_the_mirrors_have_the_c_layout(name, fields):
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


def test_bad_arguments_are_refused_before_any_launch():
    from megastep_amd import _lib
    h = _lib.lib()
    fake = 64                                       # (never dereferenced: every call below fails its checks first)
    grid = _lib.MsNavGrid(n_envs=2, cell=.125, clearance=.106, geom=fake, starts=fake, max_framed=100, free_cells=fake)
    ref = ctypes.byref

    def call(entry, struct, spec, device):
        s = struct(**spec)
        return entry(ref(grid), ref(s), None) if device else entry(ref(grid), ref(s))

    good = dict(n_fields=2, fields=fake, ids=None, n_ids=0, mask=None, labels=fake, sizes=None, reached=fake, passes=None)
    for entry, device in ((h.ms_nav_basins, True), (h.ms_host_nav_basins, False)):
        for bad in (dict(n_fields=0), dict(n_fields=-1), dict(fields=None), dict(labels=None), dict(reached=None), dict(n_ids=-1), dict(n_ids=257),
                    dict(n_ids=2), dict(sizes=fake), dict(n_ids=256, sizes=None), dict(ids=fake), dict(fields=66), dict(ids=66), dict(labels=66),
                    dict(n_ids=2, sizes=66), dict(reached=66), dict(passes=66)):
            assert call(entry, _lib.MsNavBasins, {**good, **bad}, device) == -1, bad      # (ids=fake: the labels store itself)
        assert entry(*((None, None, None) if device else (None, None))) == -1
        assert entry(*((ref(grid), None, None) if device else (ref(grid), None))) == -1
    good = dict(n_points=2, points=fake, field=None, fields=fake, labels=fake, n_fields=2, out=fake)
    for entry, device in ((h.ms_nav_basin_query, True), (h.ms_host_nav_basin_query, False)):
        for bad in (dict(n_points=0), dict(n_fields=0), dict(points=None), dict(fields=None), dict(labels=None), dict(out=None), dict(n_points=3),
                    dict(points=66), dict(field=66), dict(fields=66), dict(labels=66), dict(out=66)):
            assert call(entry, _lib.MsNavBasinQuery, {**good, **bad}, device) == -1, bad
        assert entry(*((ref(grid), None, None) if device else (ref(grid), None))) == -1
    good = dict(n_points=2, points=fake, field=None, point_ids=None, n_fields=2, marks=fake, ids=fake)
    for entry, device in ((h.ms_nav_point_marks, True), (h.ms_host_nav_point_marks, False)):
        for bad in (dict(n_points=0), dict(n_fields=0), dict(points=None), dict(marks=None), dict(ids=None), dict(n_points=3), dict(points=66),
                    dict(field=66), dict(point_ids=66), dict(ids=66)):
            assert call(entry, _lib.MsNavPointMarks, {**good, **bad}, device) == -1, bad
        assert entry(*((ref(grid), None, None) if device else (ref(grid), None))) == -1
    assert h.ms_host_nav_basin_capacity(None) == -1


def _cpu_grid():
    from megastep_amd import cuda
    geom = np.array([[0, 0, 8, 8], [0, 0, 8, 8]], np.int32)
    starts = np.array([0, 64, 128], np.int64)
    return cuda.NavGrid(torch.as_tensor(geom), torch.as_tensor(starts), torch.ones(128, dtype=torch.uint8), CELL, RADIUS, geom, starts)


def test_the_python_calls_refuse_what_they_cannot_do():
    from megastep_amd import cuda, nav
    grid = _cpu_grid()
    assert cuda.BASIN_CAPACITY is nav.BASIN_CAPACITY and cuda.basins is nav.basins and cuda.Basins is nav.Basins
    assert cuda.point_marks is nav.point_marks and cuda.PointMarks is nav.PointMarks
    points = torch.zeros((2, 2, 2))
    with pytest.raises(RuntimeError, match='GPU'):
        cuda.point_marks(grid, points)
    for bad in (0, -1, 1.5):
        with pytest.raises(RuntimeError, match='n_fields'):
            cuda.point_marks(grid, points, bad)
    for bad in (torch.zeros((3, 2, 2)), torch.zeros((2, 2, 3)), torch.zeros((2, 0, 2))):
        with pytest.raises(RuntimeError, match=r'\(N, P, 2\)'):
            cuda.point_marks(grid, bad)
    with pytest.raises(RuntimeError, match='one per point'):
        cuda.point_marks(grid, points, 3)
    for bad in (torch.zeros((2, 2)), torch.zeros((2, 3), dtype=torch.int32), torch.zeros((2, 2), dtype=torch.bool)):
        with pytest.raises(RuntimeError, match='ids must be'):
            cuda.point_marks(grid, points, ids=bad)
        with pytest.raises(RuntimeError, match='field must be'):
            cuda.point_marks(grid, points, 3, field=bad)
    marks = torch.zeros(256, dtype=torch.uint8)
    fields = cuda.SeededFields(grid, marks, 2, True, None, torch.zeros(256), torch.zeros((2, 2), dtype=torch.int32))
    with pytest.raises(RuntimeError, match='GPU'):
        cuda.basins(fields)
    with pytest.raises(RuntimeError, match='GPU'):
        fields.basins(n_ids=2)
    with pytest.raises(RuntimeError, match='four anchors'):
        cuda.basins(cuda.DistanceFields(grid, torch.zeros((2, 2, 2)), torch.zeros(256)))
    with pytest.raises(RuntimeError, match='SeededFields'):
        cuda.basins(grid)
    for bad in (-1, 257, 1.5, True):
        with pytest.raises(RuntimeError, match='n_ids'):
            cuda.basins(fields, n_ids=bad)
    for bad in (torch.zeros(256), torch.zeros((2, 128), dtype=torch.int32), torch.zeros(512, dtype=torch.int32)[::2]):
        with pytest.raises(RuntimeError, match='int32'):
            cuda.basins(fields, ids=bad)
    with pytest.raises(RuntimeError, match='entries'):
        cuda.basins(fields, ids=torch.zeros(128, dtype=torch.int32))
    ids = torch.zeros(256, dtype=torch.int32)
    new = lambda shape: torch.zeros(shape, dtype=torch.int32)
    b = cuda.Basins(fields, ids, 2, new(256), new((2, 2, 2)), new((2, 2)))
    other = cuda.SeededFields(grid, marks, 2, True, None, torch.zeros(256), torch.zeros((2, 2), dtype=torch.int32))
    for kw in (dict(fields=other), dict(ids=ids.clone()), dict(ids=None), dict(n_ids=3)):
        kw = {**dict(fields=fields, ids=ids, n_ids=2), **kw}
        with pytest.raises(RuntimeError, match='`out` must come from a basins call'):
            cuda.basins(kw.pop('fields'), **kw, out=b)
    with pytest.raises(RuntimeError, match='`out` must come from a basins call'):
        cuda.basins(fields, ids, 2, out=fields)
    for bad in (torch.ones((2, 2)), torch.ones((2, 3), dtype=torch.bool), torch.ones(4, dtype=torch.bool)):
        with pytest.raises(RuntimeError, match='mask'):
            b.update(bad)
    with pytest.raises(RuntimeError, match='GPU'):
        b.update()
    assert b.image(1, 1).shape == (8, 8) and b.image(1, 1).dtype == torch.int32 and b.n_fields == 2
    with pytest.raises(RuntimeError, match='GPU'):
        b.at(points)
    for bad in (torch.zeros((3, 2, 2)), torch.zeros((2, 2, 3)), torch.zeros((2, 0, 2))):
        with pytest.raises(RuntimeError, match=r'\(N, P, 2\)'):
            b.at(bad)
    with pytest.raises(RuntimeError, match='one per point'):
        b.at(torch.zeros((2, 3, 2)))
    with pytest.raises(RuntimeError, match='goal must be'):
        b.at(points, goal=torch.zeros((2, 2)))
    for bad in (torch.zeros((2, 2)), torch.zeros((3, 2), dtype=torch.int32), torch.zeros(2, dtype=torch.int32), torch.zeros((2, 2), dtype=torch.bool)):
        with pytest.raises(RuntimeError, match='labels must be'):
            b.masks(bad)
    with pytest.raises(RuntimeError, match='GPU'):
        b.masks(torch.zeros((2, 2), dtype=torch.int64))
    with pytest.raises(RuntimeError, match='one per point'):
        b.masks(torch.zeros((2, 3), dtype=torch.int64))


# ---------------------------------------------------------------------------------------------------------------------
# the modules' rules on CPU tensors
# ---------------------------------------------------------------------------------------------------------------------
def test_frontiers_fall_back_on_the_shared_field_and_the_expert_says_what_it_needs():
    from types import SimpleNamespace
    from megastep_amd import modules
    from megastep_amd.demo.envs.floorcoverage import FloorCoverage
    nan, inf = float('nan'), float('inf')
    own = torch.tensor([[[1., 2.], [nan, nan]], [[nan, nan], [nan, nan]], [[-3., 0.], [5., 6.]]])
    shared = torch.tensor([[[7., 7.], [8., 8.]], [[9., 9.], [nan, nan]], [[1., 1.], [2., 2.]]])
    got = modules.Frontiers.fallback(own, shared)
    assert got[0].tolist() == [[1., 2.], [8., 8.]] and got[1, 0].tolist() == [9., 9.] and torch.isnan(got[1, 1]).all()
    assert got[2].tolist() == [[-3., 0.], [5., 6.]]
    # distances: +inf is "nothing of my own left"
    got = modules.Frontiers.fallback(torch.tensor([[1., inf], [inf, 0.]]), torch.tensor([[4., 5.], [inf, 6.]]))
    assert got.tolist() == [[1., 5.], [inf, 0.]]
    with pytest.raises(RuntimeError, match='kind must be'):
        FloorCoverage.expert(None, kind='nearest')
    with pytest.raises(RuntimeError, match='shared=True'):
        FloorCoverage.expert(SimpleNamespace(_coverage=SimpleNamespace(shared=False)), 'split')
    with pytest.raises(RuntimeError, match='shared coverage'):
        modules.Frontiers(SimpleNamespace(), SimpleNamespace(shared=False), territories=object())
    for bad in (0, -2):
        with pytest.raises(RuntimeError, match='refresh'):
            modules.Territories(SimpleNamespace(), None, refresh=bad)
        with pytest.raises(RuntimeError, match='refresh'):
            modules.Frontiers(SimpleNamespace(), SimpleNamespace(shared=True), refresh=bad, territories=object())
