"""Regions (include/megastep_hip.h, MsNavRegions) restated in numpy - region_rule, a flood fill written
independently of the kernel's min-label propagation - and the host instantiations of the kernels' own per-cell functions
(ms_host_nav_regions, ms_host_nav_region_query, ms_host_nav_region_masks: csrc/kernels/navregion.h) held to EQUALITY with it. No
GPU: what is compared is the text every lane of the kernels evaluates, swept serially."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests.test_abi import ROOT, declared_symbols
from tests.test_navfield_host import CELL, CELLS, RADIUS, F, bits, nav_rule
from tests.test_navdraw_host import _aligned

NAN = F(np.nan)


class region_rule:
    """The contract in numpy and plain Python."""

    @staticmethod
    def open_cells(free, marks=None, where=True, among=None):
        """(ny, nx) bool: free (bit 0) without marks; with them MsNavSeedFields' seed predicate."""
        is_open = (np.asarray(free).astype(np.uint8) & 1) != 0
        if marks is not None:
            is_open = is_open & (((np.asarray(marks).astype(np.uint8) & 1) != 0) == bool(where))
            if among is not None:
                is_open = is_open & ((np.asarray(among).astype(np.uint8) & 1) != 0)
        return is_open

    @staticmethod
    def label(is_open):
        """(labels (ny, nx) int32, cells (ny, nx) int32) by a union-find over the rows' runs of open cells: two runs of adjacent
        rows are united when they share a column - 4-neighbours inside the grid; a run never crosses a row's end, so rows do not
        wrap. Runs are numbered in row-major order and a union keeps the lesser number, so a root is its component's first run
        and that run's first cell the component's least index."""
        ny, nx = is_open.shape
        padded = np.zeros((ny, nx + 2), np.int8)
        padded[:, 1:-1] = is_open
        step = np.diff(padded.reshape(-1))
        begin, end = np.flatnonzero(step == 1) + 1, np.flatnonzero(step == -1) + 1
        row, c0, c1 = begin//(nx + 2), begin % (nx + 2) - 1, end % (nx + 2) - 1      # (columns c0 .. c1 - 1)
        parent = list(range(len(begin)))

        def find(a):
            while parent[a] != a:
                parent[a] = parent[parent[a]]
                a = parent[a]
            return a

        first = np.searchsorted(row, np.arange(ny + 1))
        lo, hi = c0.tolist(), c1.tolist()
        for i in range(ny - 1):
            a, b, a_end, b_end = int(first[i]), int(first[i + 1]), int(first[i + 1]), int(first[i + 2])
            while a < a_end and b < b_end:
                if lo[a] < hi[b] and lo[b] < hi[a]:
                    ra, rb = find(a), find(b)
                    if ra != rb:
                        parent[max(ra, rb)] = min(ra, rb)
                if hi[a] < hi[b]:
                    a += 1
                else:
                    b += 1
        root = np.array([find(a) for a in range(len(begin))], np.int64)
        length = (c1 - c0).astype(np.int64)
        size = np.bincount(root, weights=length, minlength=len(begin)).astype(np.int64) if len(begin) else np.zeros(0, np.int64)
        label_of = (row*nx + c0)[root] if len(begin) else np.zeros(0, np.int64)
        labels, cells = np.full(is_open.shape, -1, np.int32), np.zeros(is_open.shape, np.int32)
        where = np.flatnonzero(is_open.reshape(-1))                        # (row-major: the runs one after the other)
        labels.reshape(-1)[where] = np.repeat(label_of, length)
        cells.reshape(-1)[where] = np.repeat(size[root] if len(begin) else size, length)
        return labels, cells

    @staticmethod
    def areas(cells, cell):
        return cells.astype(F)*(F(cell)*F(cell))

    @staticmethod
    def summary(labels, cells):
        """(counts, open_cells, largest, largest_cells)."""
        roots = np.flatnonzero(labels.reshape(-1) == np.arange(labels.size))
        if not len(roots):
            return 0, 0, -1, 0
        sizes = cells.reshape(-1)[roots]
        best = roots[np.flatnonzero(sizes == sizes.max())[0]]              # (roots ascend: the least label of the largest)
        return len(roots), int((labels >= 0).sum()), int(best), int(sizes.max())

    @staticmethod
    def call(geom, starts, cell, free, G=1, marks=None, where=True, among=None, mask=None, before=None):
        """One call of ms_nav_regions: dict of labels, areas (flat, the fields' layout) and the four (N, G) summaries; `before`:
        what the outputs held (masked-out fields keep it)."""
        N = len(geom)
        size = max(G*int(starts[-1]), 1)
        out = before if before is not None else dict(labels=np.full(size, -1, np.int32), areas=np.zeros(size, F), counts=np.zeros((N, G), np.int32),
                                                     open_cells=np.zeros((N, G), np.int32), largest=np.full((N, G), -1, np.int32),
                                                     largest_cells=np.zeros((N, G), np.int32))
        out = {k: np.array(v) for k, v in out.items()}
        for n in range(N):
            nx, ny = int(geom[n][2]), int(geom[n][3])
            n_cells = nx*ny if nx > 0 and ny > 0 else 0
            first = int(starts[n])
            for g in range(G):
                if mask is not None and not mask[n][g]:
                    continue
                if n_cells == 0:
                    out['counts'][n, g], out['open_cells'][n, g], out['largest'][n, g], out['largest_cells'][n, g] = 0, 0, -1, 0
                    continue
                at = G*first + g*n_cells
                take = lambda a, lo: None if a is None else np.asarray(a)[lo:lo + n_cells].reshape(ny, nx)
                is_open = region_rule.open_cells(take(free, first), take(marks, at), where, take(among, first))
                labels, cells = region_rule.label(is_open)
                out['labels'][at:at + n_cells] = labels.reshape(-1)
                out['areas'][at:at + n_cells] = region_rule.areas(cells, cell).reshape(-1)
                out['counts'][n, g], out['open_cells'][n, g], out['largest'][n, g], out['largest_cells'][n, g] = region_rule.summary(labels, cells)
        return out

    @staticmethod
    def field_of(G, P, field, n, p):
        f = int(field[n][p]) if field is not None else (0 if G == 1 else p)
        return f if 0 <= f < G else -1

    @staticmethod
    def labels_at(geom, starts, cell, labels, G, points, field=None):
        """(N, P, 4) int32: the label under each anchor of each point, in the order i0 + (t>>1), j0 + (t&1)."""
        N, P = points.shape[:2]
        out = np.full((N, P, 4), -1, np.int32)
        c = F(cell)
        for n in range(N):
            jx0, iy0, nx, ny = (int(v) for v in geom[n])
            if nx <= 0 or ny <= 0:
                continue
            for p in range(P):
                f = region_rule.field_of(G, P, field, n, p)
                with np.errstate(all='ignore'):
                    fx, fy = np.floor(F(points[n, p, 0])/c - F(.5)), np.floor(F(points[n, p, 1])/c - F(.5))
                if f < 0 or not (abs(fx) < 2.**30 and abs(fy) < 2.**30):
                    continue
                j0, i0 = int(fx) - jx0, int(fy) - iy0
                store = labels[G*int(starts[n]) + f*nx*ny:][:nx*ny].reshape(ny, nx)
                for t in range(4):
                    i, j = i0 + (t >> 1), j0 + (t & 1)
                    if 0 <= i < ny and 0 <= j < nx:
                        out[n, p, t] = store[i, j]
        return out

    @staticmethod
    def at(found):
        least = np.where(found < 0, np.iinfo(np.int32).max, found).min(-1)
        return np.where(least == np.iinfo(np.int32).max, -1, least).astype(np.int32)

    @staticmethod
    def together(la, lb):
        return ((la[..., :, None] == lb[..., None, :]) & (la[..., :, None] >= 0)).any(-1).any(-1)

    @staticmethod
    def masks(geom, starts, cell, labels, G, points=None, wanted=None, field=None):
        """P byte stores per env, the fields' layout: 1 where the cell's label is in the request's wanted set."""
        N, P = (points if points is not None else wanted).shape[:2]
        sets = region_rule.labels_at(geom, starts, cell, labels, G, points, field) if points is not None else np.asarray(wanted).reshape(N, P, 1)
        out = np.zeros(max(P*int(starts[-1]), 1), np.uint8)
        for n in range(N):
            nx, ny = int(geom[n][2]), int(geom[n][3])
            n_cells = nx*ny if nx > 0 and ny > 0 else 0
            for p in range(P):
                f = region_rule.field_of(G, P, field, n, p)
                if f < 0 or n_cells == 0:
                    continue
                store = labels[G*int(starts[n]) + f*n_cells:][:n_cells]
                want = [int(v) for v in sets[n, p] if v >= 0]
                out[P*int(starts[n]) + p*n_cells:][:n_cells] = (store >= 0) & np.isin(store, want)
        return out


# ---------------------------------------------------------------------------------------------------------------------
# the host instantiations
# ---------------------------------------------------------------------------------------------------------------------
def _max_framed(geom):
    framed = [(int(g[2]) + 2)*(int(g[3]) + 2) for g in geom if g[2] > 0 and g[3] > 0]
    return max(framed, default=0)


class _Host:
    """The three host entries on one grid of host arrays; the outputs start as sentinels."""

    def __init__(self, geom, starts, free, cell=CELL, max_framed=None, clearance=RADIUS):
        from megastep_amd import _lib
        self.geom, self.starts = _aligned(geom), np.ascontiguousarray(starts, np.int64)
        self.free = np.ascontiguousarray(np.concatenate([np.asarray(free, np.uint8).reshape(-1), np.zeros(1, np.uint8)]))
        self.N, self.cell = len(self.geom), cell
        self.grid = _lib.MsNavGrid(self.N, cell, clearance, self.geom.ctypes.data, self.starts.ctypes.data,
                                   _max_framed(self.geom) if max_framed is None else max_framed, self.free.ctypes.data)
        self.h = _lib.lib()

    def regions(self, G=1, marks=None, where=True, among=None, mask=None, before=None, passes=True):
        from megastep_amd import _lib
        size = max(G*int(self.starts[-1]), 1)
        out = before if before is not None else dict(labels=np.full(size, -7, np.int32), areas=np.full(size, F(-7), F),
                                                     **{k: np.full((self.N, G), -7, np.int32) for k in ('counts', 'open_cells', 'largest', 'largest_cells')})
        out = {k: np.ascontiguousarray(v).copy() for k, v in out.items()}
        out['passes'] = np.full((self.N, G), -7, np.int32) if passes else None
        keep = [None if a is None else np.ascontiguousarray(a, np.uint8) for a in (marks, among, mask)]
        ptr = lambda a: None if a is None else a.ctypes.data
        spec = _lib.MsNavRegions(G, ptr(keep[0]), int(bool(where)), ptr(keep[1]), ptr(keep[2]), *(out[k].ctypes.data for k in
                                 ('labels', 'areas', 'counts', 'open_cells', 'largest', 'largest_cells')), ptr(out['passes']))
        assert self.h.ms_host_nav_regions(ctypes.byref(self.grid), ctypes.byref(spec)) == 0
        return out

    def labels_at(self, labels, G, points, field=None):
        from megastep_amd import _lib
        points = np.ascontiguousarray(points, F)
        N, P = points.shape[:2]
        field = None if field is None else np.ascontiguousarray(field, np.int32)
        out = np.full((N, P, 4), -7, np.int32)
        spec = _lib.MsNavRegionQuery(P, points.ctypes.data, None if field is None else field.ctypes.data, labels.ctypes.data, G, out.ctypes.data)
        assert self.h.ms_host_nav_region_query(ctypes.byref(self.grid), ctypes.byref(spec)) == 0
        return out

    def masks(self, labels, G, points=None, wanted=None, field=None):
        from megastep_amd import _lib
        points = None if points is None else np.ascontiguousarray(points, F)
        wanted = None if wanted is None else np.ascontiguousarray(wanted, np.int32)
        field = None if field is None else np.ascontiguousarray(field, np.int32)
        P = (points if points is not None else wanted).shape[1]
        out = np.full(max(P*int(self.starts[-1]), 1), 9, np.uint8)
        ptr = lambda a: None if a is None else a.ctypes.data
        spec = _lib.MsNavRegionMasks(P, ptr(points), ptr(wanted), ptr(field), labels.ctypes.data, G, out.ctypes.data)
        assert self.h.ms_host_nav_region_masks(ctypes.byref(self.grid), ctypes.byref(spec)) == 0
        if int(self.starts[-1]) == 0:
            out[:] = 0
        return out


KEYS = ('labels', 'counts', 'open_cells', 'largest', 'largest_cells')


def same(got, want):
    """Are two results of a regions call equal - the areas as bits?"""
    for key in KEYS:
        assert np.array_equal(got[key], want[key]), (key, int((np.asarray(got[key]) != np.asarray(want[key])).sum()))
    assert np.array_equal(bits(got['areas']), bits(want['areas'])), int((bits(got['areas']) != bits(want['areas'])).sum())


# ---------------------------------------------------------------------------------------------------------------------
# hand-made grids
# ---------------------------------------------------------------------------------------------------------------------
def serpentine(side):
    """(side, side) bool: one corridor from cell (0, 0): the even rows open, joined at alternating ends."""
    m = np.zeros((side, side), bool)
    m[::2] = True
    m[1::4, -1] = True
    m[3::4, 0] = True
    return m


def comb(ny, nx):
    m = np.zeros((ny, nx), bool)
    m[0] = True
    m[:, ::2] = True
    return m


class _Hand:
    pass


_HAND = []


def hand():
    """One ragged grid of fourteen envs, see the comments; env 12 has no cells."""
    if not _HAND:
        rng = np.random.RandomState(3)
        corner = np.array([[1, 0], [0, 1]], bool)
        wrap = np.zeros((2, 4), bool)
        wrap[0, 3] = wrap[1, 0] = True
        halves = np.ones((3, 5), bool)
        halves[:, 2] = False
        envs = [((0, 0, 1, 1), np.ones((1, 1), bool)),                   # 0: 1 x 1 open
                ((4, -3, 1, 1), np.zeros((1, 1), bool)),                 # 1: 1 x 1 closed
                ((-9, 2, 70, 1), (np.arange(70) % 2 == 0)[None]),        # 2: 1 x 70 alternating
                ((-2, 3, 3, 5), rng.rand(5, 3) < .7),                    # 3: 3 x 5
                ((0, 0, 2, 2), corner),                                  # 4: two cells touching at a corner only: two regions
                ((0, 0, 2, 2), np.ones((2, 2), bool)),                   # 5: with both side cells open: one
                ((1, 1, 4, 2), wrap),                                    # 6: (0, 3) and (1, 0): rows do not wrap
                ((-16, -16, 33, 33), serpentine(33)),                    # 7: a corridor whose least index is at one end
                ((5, 5, 31, 20), comb(20, 31)),                          # 8
                ((0, -7, 11, 9), np.indices((9, 11)).sum(0) % 2 == 0),   # 9: a checkerboard: every open cell its own region
                ((-2000, 0, 64*64 + 1, 1), np.ones((1, 64*64 + 1), bool)),   # 10: 64 x 64 + 1 cells, all open
                ((3, 3, 5, 4), np.zeros((4, 5), bool)),                  # 11: none open
                ((3, 4, 0, 7), np.zeros((7, 0), bool)),                  # 12: no cells
                ((0, 0, 5, 3), halves)]                                  # 13: two regions of six cells: the least label is the largest
        w = _Hand()
        w.geom = np.array([g for g, _ in envs], np.int32)
        w.images = [m for _, m in envs]
        w.starts = np.concatenate([[0], np.cumsum([m.size for m in w.images])]).astype(np.int64)
        w.free = np.concatenate([m.reshape(-1) for m in w.images]).astype(np.uint8)
        w.free[w.free != 0] = rng.choice(np.array([1, 3, 255], np.uint8), int((w.free != 0).sum()))      # (bit 0 is what counts)
        w.free[w.starts[11]:w.starts[12]] = 2                            # (bit 0 clear: closed)
        w.N, w.n_cells = len(envs), int(w.starts[-1])
        _HAND.append(w)
    return _HAND[0]


@pytest.mark.parametrize('launch', ['fits', 'smallest'])
def test_the_free_cells_of_the_hand_made_grids(launch):
    w = hand()
    host = _Host(w.geom, w.starts, w.free, max_framed=None if launch == 'fits' else 0)       # (smallest: env 10 is labelled as stored)
    got = host.regions()
    want = region_rule.call(w.geom, w.starts, CELL, w.free)
    same(got, want)
    c = want['counts'][:, 0].tolist()
    assert c == [1, 0, 35, c[3], 2, 1, 2, 1, 1, 50, 1, 0, 0, 2]
    assert want['largest'][:, 0].tolist()[:3] == [0, -1, 0] and want['largest'][[7, 10, 11, 12, 13], 0].tolist() == [0, 0, -1, -1, 0]
    assert want['largest_cells'][[7, 10, 13], 0].tolist() == [int(serpentine(33).sum()), 64*64 + 1, 6]
    assert want['open_cells'][9, 0] == 50 and want['largest_cells'][9, 0] == 1
    assert (got['passes'][[1, 11], 0] == 1).all() and got['passes'][12, 0] == 0 and (got['passes'][[0, 2, 7, 10], 0] >= 1).all()
    # the areas are the two binary32 multiplications
    at = int(w.starts[7])
    n = int(serpentine(33).sum())
    assert bits(got['areas'][at:at + 1])[0] == bits(np.array([np.float32(n)*(np.float32(CELL)*np.float32(CELL))]))[0]
    assert (got['areas'][w.starts[11]:w.starts[12]] == 0).all() and (got['labels'][w.starts[11]:w.starts[12]] == -1).all()


@pytest.mark.parametrize('among', [False, True])
@pytest.mark.parametrize('where', [True, False])
def test_two_marked_fields_an_env_with_and_without_among_one_field_masked_out(where, among):
    w = hand()
    rng = np.random.RandomState(17 + 2*where + among)
    marks = np.empty(2*w.n_cells, np.uint8)
    for n in range(w.N):                             # (field 0: every mark set - the free cells, or nothing; field 1: random bytes)
        first, size = int(w.starts[n]), int(w.starts[n + 1] - w.starts[n])
        marks[2*first:2*first + size] = rng.choice(np.array([1, 3], np.uint8), size)
        marks[2*first + size:2*first + 2*size] = rng.choice(np.array([0, 1, 2, 3, 255], np.uint8), size)
    limit = (rng.rand(w.n_cells) < .85).astype(np.uint8)*3 if among else None
    mask = np.ones((w.N, 2), np.uint8)
    mask[7, 1] = mask[3, 0] = 0
    host = _Host(w.geom, w.starts, w.free)
    got = host.regions(2, marks, where, limit, mask)
    before = {k: np.full_like(got[k], -7) for k in KEYS + ('areas',)}
    want = region_rule.call(w.geom, w.starts, CELL, w.free, 2, marks, where, limit, mask, before)
    same(got, want)
    assert got['counts'][7, 1] == -7 and got['passes'][7, 1] == -7 and got['largest'][3, 0] == -7         # (sentinels kept)
    at = 2*int(w.starts[7]) + 33*33
    assert (got['labels'][at:at + 33*33] == -7).all() and (got['areas'][at:at + 33*33] == -7).all()
    if where and not among:
        assert got['counts'][:, 0].tolist()[4:7] == [2, 1, 2] and got['counts'][7, 0] == 1
    if not where:
        assert (got['open_cells'][:, 0][mask[:, 0] != 0] == 0).all()
    assert (want['counts'][[8, 9, 10], 1] > 1).all()


def test_fields_too_large_for_the_launch_are_labelled_as_stored_to_the_same_result():
    from megastep_amd import _lib, nav
    caps = (ctypes.c_int*3)()
    assert _lib.lib().ms_host_nav_region_capacity(caps) == 0 and tuple(caps) == nav.REGION_CAPACITY
    assert tuple(caps) == tuple((kib*1024 - 64)//4 for kib in (40, 80, 160))
    rng = np.random.RandomState(5)
    envs = [((0, 0, 101, 101), serpentine(101)), ((-50, 7, 131, 97), rng.rand(97, 131) < .62), ((3, 3, 120, 100), comb(100, 120)),
            ((0, 0, 110, 100), np.indices((100, 110)).sum(0) % 2 == 0), ((0, 0, 7, 5), np.ones((5, 7), bool))]
    geom = np.array([g for g, _ in envs], np.int32)
    assert all((g[2] + 2)*(g[3] + 2) > caps[0] for g in geom[:4]) and _max_framed(geom) <= caps[1]
    starts = np.concatenate([[0], np.cumsum([m.size for _, m in envs])]).astype(np.int64)
    free = np.concatenate([m.reshape(-1) for _, m in envs]).astype(np.uint8)
    want = region_rule.call(geom, starts, CELL, free)
    framed = _Host(geom, starts, free).regions()
    stored = _Host(geom, starts, free, max_framed=0).regions()
    same(framed, want)
    same(stored, want)
    assert want['counts'][:, 0].tolist()[0] == 1 and want['counts'][2, 0] == 1 and want['counts'][3, 0] == 5500 and want['counts'][1, 0] > 20
    # the jump: half the rows of the corridor run against the sweep; one cell a pass would be more than 2 500 passes
    print('passes, framed and stored:', framed['passes'].reshape(-1).tolist(), stored['passes'].reshape(-1).tolist())
    corridor = int(serpentine(101).sum())
    assert corridor > 5000 and 1 <= framed['passes'][0, 0] < corridor//10 and 1 <= stored['passes'][0, 0] < corridor//10


# ---------------------------------------------------------------------------------------------------------------------
# queries and masks
# ---------------------------------------------------------------------------------------------------------------------
def _centre(w, n, i, j, di=0., dj=0.):
    jx0, iy0 = int(w.geom[n][0]), int(w.geom[n][1])
    return [(jx0 + j + .5 + dj)*CELL, (iy0 + i + .5 + di)*CELL]


def test_a_point_between_two_diagonal_cells_has_two_labels_and_odd_points_have_none():
    w = hand()
    host = _Host(w.geom, w.starts, w.free)
    labels = host.regions()['labels']
    points = np.zeros((w.N, 4, 2), F)
    points[:, 0] = [_centre(w, n, 0, 0, .5, .5) for n in range(w.N)]      # (the corner the first four cells share)
    points[:, 1] = [_centre(w, n, 0, 0) for n in range(w.N)]
    points[:, 2] = NAN
    points[:, 3] = [F(2.**31), 0.]                                      # (beyond 2^30 cells of 0.125 m)
    points[9, 3] = [0., F(-np.inf)]
    got = host.labels_at(labels, 1, points, field=np.zeros((w.N, 4), np.int32))
    want = region_rule.labels_at(w.geom, w.starts, CELL, labels, 1, points, np.zeros((w.N, 4), np.int32))
    assert np.array_equal(got, want)
    assert got[4, 0].tolist() == [0, -1, -1, 3] and got[5, 0].tolist() == [0, 0, 0, 0] and got[6, 0].tolist() == [-1, -1, 4, -1]
    assert got[0, 0].tolist() == [0, -1, -1, -1] and (got[[1, 11, 12]] == -1).all() and (got[:, 2:] == -1).all()
    assert region_rule.at(got)[4].tolist() == [0, 0, -1, -1] and region_rule.at(got)[6, 0] == 4
    # the default field with one regions field, and a field index of -1 and of G
    assert np.array_equal(host.labels_at(labels, 1, points), want)
    field = np.zeros((w.N, 4), np.int32)
    field[:, 0], field[:, 1] = -1, 1
    odd = host.labels_at(labels, 1, points, field=field)
    assert (odd == -1).all() and np.array_equal(odd, region_rule.labels_at(w.geom, w.starts, CELL, labels, 1, points, field))


def test_fields_given_and_defaulted_with_one_field_per_point():
    w = hand()
    rng = np.random.RandomState(2)
    marks = rng.choice(np.array([0, 1, 1, 3], np.uint8), 3*w.n_cells)
    host = _Host(w.geom, w.starts, w.free)
    labels = host.regions(3, marks)['labels']
    points = np.array([[_centre(w, n, rng.randint(0, max(w.geom[n][3], 1)), rng.randint(0, max(w.geom[n][2], 1)), *rng.uniform(-.5, .5, 2))
                        for _ in range(3)] for n in range(w.N)], F)
    got = host.labels_at(labels, 3, points)
    assert np.array_equal(got, region_rule.labels_at(w.geom, w.starts, CELL, labels, 3, points))
    assert np.array_equal(got, host.labels_at(labels, 3, points, field=np.tile(np.arange(3, dtype=np.int32), (w.N, 1))))
    assert (got >= 0).sum() > 40
    field = rng.randint(-1, 4, (w.N, 3))
    got = host.labels_at(labels, 3, points, field=field)
    assert np.array_equal(got, region_rule.labels_at(w.geom, w.starts, CELL, labels, 3, points, field))
    assert (got[(field < 0) | (field > 2)] == -1).all()
    for kw in (dict(points=points), dict(points=points, field=field), dict(wanted=got[..., 0]), dict(wanted=got[..., 3], field=field)):
        assert np.array_equal(host.masks(labels, 3, **kw), region_rule.masks(w.geom, w.starts, CELL, labels, 3, **kw)), list(kw)


def test_masks_by_a_straddling_point_are_two_regions_and_the_mask_of_minus_one_is_empty():
    w = hand()
    host = _Host(w.geom, w.starts, w.free)
    labels = host.regions()['labels']
    points = np.array([[_centre(w, n, 0, 0, .5, .5)] for n in range(w.N)], F)
    got = host.masks(labels, 1, points=points)
    assert np.array_equal(got, region_rule.masks(w.geom, w.starts, CELL, labels, 1, points=points))
    assert got[w.starts[4]:w.starts[5]].tolist() == [1, 0, 0, 1] and got[w.starts[6]:w.starts[7]].tolist() == [0, 0, 0, 0, 1, 0, 0, 0]
    assert got[w.starts[13]:w.starts[14]].tolist() == [1, 1, 0, 0, 0]*3 and got.max() == 1
    wanted = np.full((w.N, 2), -1, np.int32)
    wanted[:, 1] = [0, 0, 4, 0, 3, 0, 4, 0, 0, 2, 0, 0, 0, 3]
    got = host.masks(labels, 1, wanted=wanted)
    assert np.array_equal(got, region_rule.masks(w.geom, w.starts, CELL, labels, 1, wanted=wanted))
    for n in range(w.N):
        first, size = int(w.starts[n]), int(w.starts[n + 1] - w.starts[n])
        assert not got[2*first:2*first + size].any()                     # (-1: nothing, closed cells included)
        second = got[2*first + size:2*first + 2*size]
        assert np.array_equal(second, (labels[first:first + size] == wanted[n, 1]).astype(np.uint8))
    assert got[2*w.starts[13] + 15:][:15].tolist() == [0, 0, 0, 1, 1]*3 and got[2*w.starts[4] + 4:][:4].tolist() == [0, 0, 0, 1]


# ---------------------------------------------------------------------------------------------------------------------
# real plans
# ---------------------------------------------------------------------------------------------------------------------
_PLANS = {}


def plan_regions(cell=CELL, r=RADIUS):
    """test_navdraw_host's plan_world - the six plans as one grid, and the rule's field round each plan's first viewer - with the
    host's regions of it and the rule's: (geom, starts, free, D, host, got, want)."""
    if (cell, r) not in _PLANS:
        from tests.test_navdraw_host import plan_world
        geom, starts, free, D = plan_world(cell, r)
        host = _Host(geom, starts, free, cell=cell, clearance=r)
        _PLANS[cell, r] = (geom, starts, free, D, host, host.regions(), region_rule.call(geom, starts, cell, free))
    return _PLANS[cell, r]


@pytest.mark.parametrize('cell,r', CELLS)
def test_on_the_six_plans_the_labels_areas_masks_and_pairs_are_the_rules_at_other_cell_widths(cell, r):
    """Labels and float areas - cells*(c*c), rounded when the cell is no power of two - then the labels at points, the mask of a
    point and whether two points are together, each against the rule and against the distance field's finiteness."""
    from tests.test_navseen_host import cases
    geom, starts, free, D, host, got, want = plan_regions(cell, r)
    same(got, want)
    assert (want['counts'] >= 1).all() and (want['largest_cells'] > 500*(CELL/cell)**2).all() and (got['passes'] >= 1).all()
    cs = cases(cell, r)
    points = np.stack([c.origins[:1] for c in cs]).astype(F)
    masks = host.masks(got['labels'], 1, points=points)
    assert np.array_equal(masks, region_rule.masks(geom, starts, cell, want['labels'], 1, points=points))
    assert np.array_equal(masks[:len(D)], np.isfinite(D).astype(np.uint8)) and masks.sum() > 3000*(CELL/cell)**2
    rng = np.random.RandomState(13)
    a = np.stack([c.origins[0] + rng.uniform(-3., 3., (32, 2)) for c in cs]).astype(F)
    b = np.repeat(points, 32, 1)
    la = host.labels_at(got['labels'], 1, a)
    assert np.array_equal(la, region_rule.labels_at(geom, starts, cell, want['labels'], 1, a)) and (la >= 0).any(-1).mean() > .5
    finite = np.array([[np.isfinite(nav_rule.query(D[starts[n]:starts[n + 1]].reshape(c.free.shape), c.geom, cell, c.free, p)) for p in a[n]]
                       for n, c in enumerate(cs)])
    assert np.array_equal(region_rule.together(la, host.labels_at(got['labels'], 1, b)), finite) and finite.any() and (~finite).any()


def test_on_the_six_plans_the_labels_are_the_rules():
    geom, starts, free, D, host, got, want = plan_regions()
    same(got, want)
    assert (want['counts'] >= 1).all() and (want['largest_cells'] > 500).all() and (got['passes'] >= 1).all()
    print('passes of the serial sweeps on the six plans:', got['passes'].reshape(-1).tolist())


def test_on_the_six_plans_the_counts_are_scipys():
    ndimage = pytest.importorskip('scipy.ndimage')
    geom, starts, free, D, host, got, want = plan_regions()
    cross = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]])
    for n in range(len(geom)):
        image = free[starts[n]:starts[n + 1]].reshape(geom[n][3], geom[n][2]) != 0
        assert ndimage.label(image, structure=cross)[1] == got['counts'][n, 0]


def test_on_the_six_plans_the_mask_of_a_spawn_point_is_where_its_distance_field_is_finite():
    from tests.test_navseen_host import cases
    geom, starts, free, D, host, got, want = plan_regions()
    points = np.stack([c.origins[:1] for c in cases()]).astype(F)         # (6, 1, 2): the points the fields D are of
    masks = host.masks(got['labels'], 1, points=points)
    assert np.array_equal(masks[:-1] if len(masks) > len(D) else masks, np.isfinite(D).astype(np.uint8))
    assert masks.sum() > 3000 and (masks[:len(free)] <= (free != 0)).all()


def test_on_the_six_plans_together_is_where_the_geodesic_is_finite():
    from tests.test_navseen_host import cases
    geom, starts, free, D, host, got, want = plan_regions()
    rng = np.random.RandomState(13)
    cs = cases()
    b = np.stack([np.repeat(c.origins[:1], 32, 0) for c in cs]).astype(F)     # (6, 32, 2): the point each plan's field is of
    a = np.empty_like(b)
    for n, c in enumerate(cs):
        labels = want['labels'][starts[n]:starts[n + 1]]
        home = region_rule.at(region_rule.labels_at(geom[n:n + 1], [0], CELL, labels, 1, b[n:n + 1, :1]))[0, 0]
        inside, outside = np.flatnonzero(labels == home), np.flatnonzero((labels >= 0) & (labels != home))
        # half the pairs from the point's own region, half - where the plan has another - from the others', by the rule
        cells = np.concatenate([rng.choice(inside, 16), rng.choice(outside if len(outside) else inside, 16)])
        x, y = nav_rule.centres(tuple(geom[n]), CELL)
        a[n, :, 0], a[n, :, 1] = x[cells % geom[n][2]], y[cells//geom[n][2]]
        a[n] += rng.uniform(-.4, .4, (32, 2)).astype(F)*F(CELL)
    la, lb = host.labels_at(got['labels'], 1, a), host.labels_at(got['labels'], 1, b)
    together = region_rule.together(la, lb)
    finite = np.empty((len(cs), 32), bool)
    for n, c in enumerate(cs):
        field = D[starts[n]:starts[n + 1]].reshape(c.free.shape)
        finite[n] = [np.isfinite(nav_rule.query(field, c.geom, CELL, c.free, p)) for p in a[n]]
    assert np.array_equal(together, finite)
    assert together.any() and (~together).any()                          # (both outcomes occur)


# ---------------------------------------------------------------------------------------------------------------------
# frontier regions
# ---------------------------------------------------------------------------------------------------------------------
def test_the_open_cells_of_frontier_regions_are_the_seeds_of_the_frontier_fields():
    from tests.test_navwindow_host import world
    from tests.test_navseed_host import host_field
    w = world()
    host = _Host(w.geom, w.starts, w.free[:int(w.starts[-1])])
    for among in (None, (np.random.RandomState(4).rand(int(w.starts[-1]) + 1) < .7).astype(np.uint8)):
        got = host.regions(2, w.seen, where=False, among=among)
        same(got, region_rule.call(w.geom, w.starts, CELL, w.free, 2, w.seen, False, among))
        for n in range(len(w.geom)):
            nx, ny = int(w.geom[n][2]), int(w.geom[n][3])
            first, size = int(w.starts[n]), nx*ny
            for s in range(2):
                if size == 0:
                    assert got['open_cells'][n, s] == 0
                    continue
                at = 2*first + s*size
                D, n_seeds, _ = host_field(w.geom[n], CELL, w.free[first:first + size].reshape(ny, nx), w.seen[at:at + size].reshape(ny, nx), 0,
                                           None if among is None else among[first:first + size].reshape(ny, nx), framed=1)
                assert got['open_cells'][n, s] == n_seeds
                zero = bits(D) == 0                                      # (+0.f: exactly the seeds)
                assert np.array_equal(got['labels'][at:at + size].reshape(ny, nx) >= 0, zero)
                if among is None:
                    assert np.array_equal(zero.reshape(-1), bits(w.fields[at:at + size]) == 0)
    assert (got['open_cells'][:6] > 0).all() and (got['counts'][:6] > 1).any()


# ---------------------------------------------------------------------------------------------------------------------
# header, loader, refusals
# ---------------------------------------------------------------------------------------------------------------------
ENTRIES = {'ms_nav_regions', 'ms_nav_region_query', 'ms_nav_region_masks'}
HOOKS = {'ms_host_nav_regions', 'ms_host_nav_region_query', 'ms_host_nav_region_masks', 'ms_host_nav_region_capacity'}


def test_the_header_declares_the_calls_and_the_abi_version_stays():
    from megastep_amd import _lib
    assert ENTRIES <= set(declared_symbols(('megastep_hip.h',))) and HOOKS <= set(declared_symbols(('megastep_hip_test.h',)))
    assert ENTRIES | HOOKS <= set(_lib.SYMBOLS)
    text = open(os.path.join(ROOT, 'include', 'megastep_hip.h')).read()
    assert int(re.search(r'#define MS_ABI_VERSION (\d+)', text).group(1)) == _lib.ABI_VERSION == 17
    handle = _lib.lib()
    assert all(hasattr(handle, name) for name in ENTRIES | HOOKS)


@pytest.mark.parametrize('name, fields', [
    ('MsNavRegions', ('n_fields', 'marks', 'where', 'among', 'mask', 'labels', 'areas', 'counts', 'open_cells', 'largest', 'largest_cells', 'passes')),
    ('MsNavRegionQuery', ('n_points', 'points', 'field', 'labels', 'n_fields', 'labels_at')),
    ('MsNavRegionMasks', ('n_requests', 'points', 'wanted', 'field', 'labels', 'n_fields', 'out'))])
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

    good = dict(n_fields=2, marks=fake, where=1, among=None, mask=None, labels=fake, areas=fake, counts=fake, open_cells=fake, largest=fake,
                largest_cells=fake, passes=None)
    for entry, device in ((h.ms_nav_regions, True), (h.ms_host_nav_regions, False)):
        for bad in (dict(n_fields=0), dict(n_fields=-1), dict(where=2), dict(where=-1), dict(labels=None), dict(areas=None), dict(counts=None),
                    dict(open_cells=None), dict(largest=None), dict(largest_cells=None), dict(labels=66), dict(areas=66), dict(counts=66),
                    dict(open_cells=66), dict(largest=66), dict(largest_cells=66), dict(passes=66)):
            assert call(entry, _lib.MsNavRegions, {**good, **bad}, device) == -1, bad
        assert entry(*((None, None, None) if device else (None, None))) == -1
        assert entry(*((ref(grid), None, None) if device else (ref(grid), None))) == -1
    good = dict(n_points=2, points=fake, field=None, labels=fake, n_fields=2, labels_at=fake)
    for entry, device in ((h.ms_nav_region_query, True), (h.ms_host_nav_region_query, False)):
        for bad in (dict(n_points=0), dict(n_fields=0), dict(points=None), dict(labels=None), dict(labels_at=None), dict(n_points=3),
                    dict(points=66), dict(field=66), dict(labels=66), dict(labels_at=66)):
            assert call(entry, _lib.MsNavRegionQuery, {**good, **bad}, device) == -1, bad
    good = dict(n_requests=2, points=fake, wanted=None, field=None, labels=fake, n_fields=2, out=fake)
    for entry, device in ((h.ms_nav_region_masks, True), (h.ms_host_nav_region_masks, False)):
        for bad in (dict(n_requests=0), dict(n_fields=0), dict(points=None), dict(wanted=fake), dict(labels=None), dict(out=None), dict(n_requests=3),
                    dict(points=66), dict(points=None, wanted=66), dict(field=66), dict(labels=66)):
            assert call(entry, _lib.MsNavRegionMasks, {**good, **bad}, device) == -1, bad


def test_the_python_calls_refuse_what_they_cannot_do():
    from megastep_amd import cuda, nav
    from megastep_amd.demo.envs import pointgoal
    geom = np.array([[0, 0, 8, 8], [0, 0, 8, 8]], np.int32)
    starts = np.array([0, 64, 128], np.int64)
    grid = cuda.NavGrid(torch.as_tensor(geom), torch.as_tensor(starts), torch.ones(128, dtype=torch.uint8), CELL, RADIUS, geom, starts)
    marks = torch.zeros(256, dtype=torch.uint8)
    assert cuda.REGION_CAPACITY is nav.REGION_CAPACITY and cuda.regions is nav.regions and cuda.Regions is nav.Regions
    with pytest.raises(RuntimeError, match='GPU'):
        cuda.regions(grid)                           # (CPU tensors)
    with pytest.raises(RuntimeError, match='GPU'):
        cuda.regions(grid, marks, 2)
    for bad in (0, -1, 1.5):
        with pytest.raises(RuntimeError, match='n_fields'):
            cuda.regions(grid, marks, bad)
    with pytest.raises(RuntimeError, match='entries'):
        cuda.regions(grid, marks, 3)
    with pytest.raises(RuntimeError, match='uint8 or bool'):
        cuda.regions(grid, marks.float(), 2)
    with pytest.raises(RuntimeError, match='uint8 or bool'):
        cuda.regions(grid, marks.reshape(2, 128), 2)
    with pytest.raises(RuntimeError, match='among'):
        cuda.regions(grid, among=torch.ones(128, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match='entries'):
        cuda.regions(grid, marks, 2, among=torch.ones(100, dtype=torch.uint8))
    new = lambda shape, dtype: torch.zeros(shape, dtype=dtype)
    r = cuda.Regions(grid, marks, 2, True, None, new(256, torch.int32), new(256, torch.float32), *(new((2, 2), torch.int32) for _ in range(4)))
    for other in (dict(grid=cuda.NavGrid(torch.as_tensor(geom), torch.as_tensor(starts), torch.ones(128, dtype=torch.uint8), CELL, RADIUS, geom, starts)),
                  dict(marks=marks.clone()), dict(n_fields=1, marks=marks[:128]), dict(where=False), dict(among=torch.ones(128, dtype=torch.uint8)),
                  dict(marks=None, n_fields=1)):
        kw = {**dict(grid=grid, marks=marks, n_fields=2, where=True, among=None), **other}
        with pytest.raises(RuntimeError, match='`out` must come from a regions call'):
            cuda.regions(kw.pop('grid'), **kw, out=r)
    with pytest.raises(RuntimeError, match='`out` must come from a regions call'):
        cuda.regions(grid, marks, 2, out=cuda.seeded_fields)
    for bad in (torch.ones((2, 2)), torch.ones((2, 3), dtype=torch.bool), torch.ones(4, dtype=torch.bool)):
        with pytest.raises(RuntimeError, match='mask'):
            r.update(bad)
    with pytest.raises(RuntimeError, match='GPU'):
        r.update()
    points = torch.zeros((2, 2, 2))
    with pytest.raises(RuntimeError, match='GPU'):
        r.labels_at(points)
    for bad in (torch.zeros((3, 2, 2)), torch.zeros((2, 2, 3)), torch.zeros((2, 0, 2))):
        with pytest.raises(RuntimeError, match=r'\(N, P, 2\)'):
            r.labels_at(bad)
    with pytest.raises(RuntimeError):
        r.labels_at(points.double())
    with pytest.raises(RuntimeError, match='one per point'):
        r.labels_at(torch.zeros((2, 3, 2)))
    for bad in (torch.zeros((2, 3)), torch.zeros((2, 2), dtype=torch.long), torch.zeros((2, 3), dtype=torch.bool)):
        with pytest.raises(RuntimeError, match='field'):
            r.at(torch.zeros((2, 3, 2)), field=bad)
    with pytest.raises(RuntimeError, match='field'):
        r.together(points, points, field=torch.zeros((2, 2)))
    for kw in (dict(), dict(points=points, labels=torch.zeros((2, 2), dtype=torch.int32))):
        with pytest.raises(RuntimeError, match='exactly one'):
            r.masks(**kw)
    for bad in (torch.zeros((2, 2)), torch.zeros((3, 2), dtype=torch.int32), torch.zeros(2, dtype=torch.int32), torch.zeros((2, 2), dtype=torch.bool)):
        with pytest.raises(RuntimeError, match='labels must be'):
            r.masks(labels=bad)
    with pytest.raises(RuntimeError, match='GPU'):
        r.masks(points=points)
    with pytest.raises(RuntimeError, match='one regions field per env'):
        r.largest_mask()
    layer = cuda.cell_layer(r)
    assert layer.values is r.areas and layer.n_fields == 2 and layer.is_float
    assert cuda.map_channel(r, scale=.1).source.values is r.areas
    maps = cuda.seen_maps(grid, 2)
    with pytest.raises(RuntimeError, match='GPU'):
        maps.frontier_regions()
    with pytest.raises(RuntimeError, match='sampled_spawns'):
        pointgoal.PointGoal(2, one_region=True, device='cpu', geometries=[])
