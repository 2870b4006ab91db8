"""Zones (include/megastep_hip.h, MsNavZones) restated in numpy and plain Python - zone_rule: loops over cells, a
Python min over (value bits, cell), written apart from the kernel's text - and the host instantiation of the kernel's own per-cell
functions (ms_host_nav_zones: csrc/kernels/navzone.h) held to EQUALITY with it, every output of every case. No GPU: what is compared
is the text every lane of the kernel evaluates, swept serially. Assignments.choose, the pure-torch rule on top, against a Python loop."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch

from tests.test_abi import ROOT, declared_symbols
from tests.test_navfield_host import CELL, F, INF, bits, nav_rule
from tests.test_navbasin_host import _BasinHost, _cpu_grid, plan_world

NAN = F(np.nan)
KEYS = ('cells', 'marked', 'least', 'nearest', 'points', 'roots', 'n_zones')


def zone_rule(geom, starts, cell, labels, L, n_fields, K, ranked, values=None, V=1, marks=None, M=1, where=True, within=False, mask=None,
              before=None):
    """One call of ms_nav_zones: dict of the seven outputs. `before`: what they held (masked-out fields keep it)."""
    N = len(geom)
    shape = (N, n_fields, K)
    out = before if before is not None else dict(cells=np.zeros(shape, np.int32), marked=np.zeros(shape, np.int32), least=np.full(shape, INF, F),
                                                 nearest=np.full(shape, -1, np.int32), points=np.full(shape + (2,), NAN, F),
                                                 roots=np.full(shape, -1, np.int32), n_zones=np.zeros(shape[:2], np.int32))
    out = {k: np.array(v) for k, v in out.items()}
    for n in range(N):
        jx0, iy0, nx, ny = (int(v) for v in geom[n])
        cells = nx*ny if nx > 0 and ny > 0 else 0
        s = int(starts[n])
        for f in range(n_fields):
            if mask is not None and not mask[n][f]:
                continue
            store = lambda a, count: np.asarray(a)[count*s + (0 if count == 1 else f)*cells:][:cells]
            count, marked, best, roots, total = [0]*K, [0]*K, [None]*K, [-1]*K, 0
            if cells:
                lab = store(labels, L).tolist()
                val = None if values is None else bits(store(values, V)).tolist()
                mk = None if marks is None else store(marks, M).tolist()
                if ranked:
                    every = [v for v in range(cells) if lab[v] == v]
                    total = len(every)
                    rank = {r: k for k, r in enumerate(every[:K])}
                    roots[:len(rank)] = every[:K]
                for v in range(cells):
                    k = rank.get(lab[v], -1) if ranked else (lab[v] if 0 <= lab[v] < K else -1)
                    if k < 0:
                        continue
                    count[k] += 1
                    m = True if mk is None else ((mk[v] != 0) == bool(where))
                    marked[k] += m
                    if val is not None and (m or not within) and val[v] < 0x7f800000:       # (sign bit clear and below +inf)
                        key = (val[v], v)
                        best[k] = key if best[k] is None else min(best[k], key)
                if not ranked:
                    roots = [k if count[k] > 0 else -1 for k in range(K)]
                    total = sum(c > 0 for c in count)
            out['cells'][n, f], out['marked'][n, f], out['roots'][n, f], out['n_zones'][n, f] = count, marked, roots, total
            for k in range(K):
                if best[k] is None:
                    out['least'][n, f, k], out['nearest'][n, f, k], out['points'][n, f, k] = INF, -1, NAN
                else:
                    b, v = best[k]
                    i, j = divmod(v, nx)
                    out['least'][n, f, k] = np.array([b], np.uint32).view(F)[0]
                    out['nearest'][n, f, k] = v
                    out['points'][n, f, k] = [(F(jx0 + j) + F(.5))*F(cell), (F(iy0 + i) + F(.5))*F(cell)]
    return out


class _ZoneHost(_BasinHost):
    """ms_host_nav_zones (and, inherited, the regions' and basins' host entries) on one grid of host arrays; the outputs start as
    sentinels."""

    def zones(self, labels, L, n_fields, K, ranked, values=None, V=1, marks=None, M=1, where=True, within=False, mask=None, before=None,
              status=0):
        from megastep_amd import _lib
        shape = (self.N, n_fields, K)
        out = before if before is not None else dict(cells=np.full(shape, -7, np.int32), marked=np.full(shape, -7, np.int32),
                                                     least=np.full(shape, -7, F), nearest=np.full(shape, -7, np.int32),
                                                     points=np.full(shape + (2,), -7, F), roots=np.full(shape, -7, np.int32),
                                                     n_zones=np.full(shape[:2], -7, np.int32))
        out = {k: np.ascontiguousarray(v).copy() for k, v in out.items()}
        pad = lambda a, dtype: None if a is None else np.ascontiguousarray(np.concatenate([np.asarray(a, dtype).reshape(-1), np.zeros(1, dtype)]))
        labels, values, marks = pad(labels, np.int32), pad(values, F), pad(marks, np.uint8)
        mask = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        ptr = lambda a: None if a is None else a.ctypes.data
        spec = _lib.MsNavZones(n_fields, ptr(labels), L, ptr(values), V, ptr(marks), M, int(bool(where)), int(bool(within)), int(bool(ranked)), K,
                               ptr(mask), *(out[k].ctypes.data for k in KEYS))
        assert self.h.ms_host_nav_zones(ctypes.byref(self.grid), ctypes.byref(spec)) == status
        return out


def same(got, want):
    for key in ('cells', 'marked', 'nearest', 'roots', 'n_zones'):
        assert np.array_equal(got[key], want[key]), (key, int((np.asarray(got[key]) != np.asarray(want[key])).sum()))
    assert np.array_equal(bits(got['least']), bits(want['least'])), 'least'
    assert np.array_equal(got['points'], want['points'], equal_nan=True), 'points'


# ---------------------------------------------------------------------------------------------------------------------
# hand-made grids
# ---------------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (5, 3), (0, 4), (3, 5), (63, 1), (64, 1), (65, 1), (255, 1), (256, 1), (257, 1), (23, 17), (4, 0), (300, 3)]      # (nx, ny)
EMPTY = (2, 11)                                     # the envs without cells: between envs that have some


class _Hand:
    def __init__(self):
        self.geom = np.array([(3*n - 7, 5 - 2*n, nx, ny) for n, (nx, ny) in enumerate(SHAPES)], np.int32)
        self.sizes = [nx*ny for nx, ny in SHAPES]
        self.starts = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)
        self.N, self.n_cells = len(SHAPES), int(self.starts[-1])
        self.free = np.ones(self.n_cells, np.uint8)

    def host(self):
        return _ZoneHost(self.geom, self.starts, self.free)

    def layer(self, make, count):
        """A flat layer of `count` stores per env in the fields' layout: make(n, cells) gives one store's entries."""
        return np.concatenate([make(n, c) for n, c in enumerate(self.sizes) for _ in range(count)] + [make(0, 0)])

    def at(self, n, count=1, f=0):
        return count*int(self.starts[n]) + f*self.sizes[n]


_HAND = []


def hand():
    if not _HAND:
        _HAND.append(_Hand())
    return _HAND[0]


def ranked_labels(rng, n_roots):
    """make(n, cells) of labels as a regions call could leave them, and as it could not: `n_roots` (at most) cells name themselves;
    the others name a root, -1, another negative, a cell that is no root, or something beyond the env."""
    def make(n, cells):
        if cells == 0:
            return np.zeros(0, np.int32)
        roots = np.sort(rng.choice(cells, min(n_roots, cells), replace=False))
        others = np.setdiff1d(np.arange(cells), roots)
        pool = np.concatenate([np.repeat(roots, 6), [-1, -5, cells, cells + 9, 2**31 - 1], others[:2]])
        lab = rng.choice(pool, cells)
        lab[lab == np.arange(cells)] = -1                                # (no root by accident)
        lab[roots] = roots
        return lab.astype(np.int32)
    return make


def direct_labels(rng, K):
    return lambda n, cells: rng.randint(-2, K + 3, cells).astype(np.int32)


def some_values(rng):
    """A few distinct values, so that ties are the rule, and every kind that takes no part."""
    pool = np.array([0., .125, .125, .5, 1.5, 3., np.inf, np.nan, -1., -0., -np.inf, 1e-45], F)
    return lambda n, cells: rng.choice(pool, cells).astype(F)


def some_marks(rng):
    return lambda n, cells: rng.choice(np.array([0, 0, 1, 2, 255], np.uint8), cells)


def run(w, labels, L, n_fields, K, ranked, **kw):
    got = w.host().zones(labels, L, n_fields, K, ranked, **kw)
    want = zone_rule(w.geom, w.starts, CELL, labels, L, n_fields, K, ranked, **kw)
    same(got, want)
    assert np.array_equal(np.isnan(got['points']).all(-1), got['nearest'] < 0) and np.array_equal(np.isinf(got['least']), got['nearest'] < 0)
    return got


@pytest.mark.parametrize('ranked', [True, False])
@pytest.mark.parametrize('K', [1, 5, 256])
def test_the_hand_made_grids_with_values_and_marks(ranked, K):
    """1 x 1 cells, envs without cells between envs that have some, rows of 63, 64, 65 and 255, 256, 257 cells, K = 1 and 256."""
    w = hand()
    rng = np.random.RandomState(K + ranked)
    labels = w.layer(ranked_labels(rng, 7) if ranked else direct_labels(rng, K), 1)
    values, marks = w.layer(some_values(rng), 1), w.layer(some_marks(rng), 1)
    got = run(w, labels, 1, 1, K, ranked, values=values, marks=marks)
    for n in EMPTY:                                                      # (zeros, +inf, -1 and NaN)
        assert not got['cells'][n].any() and not got['marked'][n].any() and np.isinf(got['least'][n]).all() and (got['nearest'][n] == -1).all()
        assert np.isnan(got['points'][n]).all() and (got['roots'][n] == -1).all() and got['n_zones'][n, 0] == 0
    assert got['cells'].sum() > 100 and (got['marked'] <= got['cells']).all() and (got['marked'] < got['cells']).any()
    assert np.isfinite(got['least']).any() and (got['nearest'] >= 0).any()
    if ranked:
        assert got['n_zones'][[0, 1, 10], 0].tolist() == [1, 7, 7] and (got['roots'][0, 0, 1:] == -1).all()
        assert (got['n_zones'][:, 0] > K).any() == (K < 7)
    else:
        assert (got['n_zones'][:, 0] <= K).all()


def test_without_values_and_without_marks():
    w = hand()
    rng = np.random.RandomState(2)
    labels = w.layer(ranked_labels(rng, 4), 1)
    got = run(w, labels, 1, 1, 6, True)
    assert np.array_equal(got['marked'], got['cells']) and np.isinf(got['least']).all() and (got['nearest'] == -1).all() and np.isnan(got['points']).all()
    got = run(w, labels, 1, 1, 6, True, values=w.layer(some_values(rng), 1), within=True)      # (no marks: every cell is marked)
    assert np.array_equal(got['marked'], got['cells']) and np.isfinite(got['least']).any()


def test_the_only_root_at_the_last_cell():
    w = hand()
    labels = w.layer(lambda n, cells: np.full(cells, cells - 1, np.int32), 1)
    values = w.layer(lambda n, cells: np.arange(cells, 0, -1).astype(F), 1)
    got = run(w, labels, 1, 1, 3, True, values=values)
    for n, cells in enumerate(w.sizes):
        if cells:
            assert got['n_zones'][n, 0] == 1 and got['roots'][n, 0].tolist() == [cells - 1, -1, -1] and got['cells'][n, 0].tolist() == [cells, 0, 0]
            assert got['least'][n, 0, 0] == 1 and got['nearest'][n, 0, 0] == cells - 1


@pytest.mark.parametrize('n', [4, 7, 9, 12])
def test_exactly_k_roots_and_one_more(n):
    """K roots: every zone is told; K + 1: n_zones says so, and the last zone's cells appear nowhere else."""
    w = hand()
    rng = np.random.RandomState(n)
    cells = w.sizes[n]
    K = 5
    roots = np.sort(rng.choice(cells, K + 1, replace=False))
    for n_roots in (K, K + 1):
        lab = rng.choice(roots[:n_roots], cells).astype(np.int32)
        lab[roots[:n_roots]] = roots[:n_roots]
        if n_roots == K:
            lab[lab == roots[K]] = -1
        labels = w.layer(lambda m, c: lab if m == n else np.full(c, -1, np.int32), 1)
        got = run(w, labels, 1, 1, K, True, values=w.layer(some_values(rng), 1))
        assert got['n_zones'][n, 0] == n_roots and got['roots'][n, 0].tolist() == roots[:K].tolist()
        assert got['cells'][n, 0].tolist() == [int((lab == r).sum()) for r in roots[:K]]
        assert got['cells'][n, 0].sum() == cells - (int((lab == roots[K]).sum()) if n_roots > K else int((lab == -1).sum()))
        assert got['cells'].sum() == got['cells'][n, 0].sum()


def test_every_cell_its_own_root_at_the_most_zones():
    w = hand()
    labels = w.layer(lambda n, cells: np.arange(cells, dtype=np.int32), 1)
    values = w.layer(lambda n, cells: (np.arange(cells) % 7).astype(F), 1)
    got = run(w, labels, 1, 1, 256, True, values=values)
    assert got['n_zones'][:, 0].tolist() == w.sizes
    assert (got['cells'][9, 0] == 1).all() and got['nearest'][9, 0].tolist() == list(range(256)) and got['cells'][12, 0].sum() == 256
    got = run(w, labels, 1, 1, 1, True, values=values)
    assert got['cells'][:, 0, 0].tolist() == [min(c, 1) for c in w.sizes]


def test_of_equal_values_the_least_index_wins():
    w = hand()
    labels = w.layer(lambda n, cells: np.zeros(cells, np.int32), 1)
    def values(n, cells):
        v = np.full(cells, 2., F)
        v[cells//3:] = .25                                               # (every cell from there on attains the least)
        v[-1:] = .25
        return v
    got = run(w, labels, 1, 1, 2, False, values=w.layer(values, 1))
    for n, cells in enumerate(w.sizes):
        if cells:
            assert got['nearest'][n, 0].tolist() == [cells//3, -1] and got['least'][n, 0, 0] == .25
    n, nx = 10, SHAPES[10][0]
    i, j = divmod(w.sizes[n]//3, nx)
    assert got['points'][n, 0, 0].tolist() == [(F(int(w.geom[n][0]) + j) + F(.5))*F(CELL), (F(int(w.geom[n][1]) + i) + F(.5))*F(CELL)]


def test_a_zone_whose_values_all_take_no_part():
    w = hand()
    labels = w.layer(lambda n, cells: (np.arange(cells) % 2).astype(np.int32), 1)
    bad = np.array([np.inf, np.nan, -1., -0., -np.inf, -1e-45], F)
    def values(n, cells):
        v = np.resize(bad, cells)
        v[1::2] = 1.                                                     # (zone 1: ordinary)
        return v
    got = run(w, labels, 1, 1, 2, False, values=w.layer(values, 1))
    has = np.array(w.sizes) > 0
    assert np.isinf(got['least'][has, 0, 0]).all() and (got['nearest'][:, 0, 0] == -1).all() and np.isnan(got['points'][:, 0, 0]).all()
    assert (got['cells'][has, 0, 0] > 0).all() and (got['least'][np.array(w.sizes) > 1, 0, 1] == 1).all()


@pytest.mark.parametrize('where', [True, False])
@pytest.mark.parametrize('within', [True, False])
def test_where_and_within_marks(where, within):
    w = hand()
    rng = np.random.RandomState(11)
    labels, values, marks = w.layer(direct_labels(rng, 4), 1), w.layer(some_values(rng), 1), w.layer(some_marks(rng), 1)
    got = run(w, labels, 1, 1, 4, False, values=values, marks=marks, where=where, within=within)
    other = run(w, labels, 1, 1, 4, False, values=values, marks=marks, where=not where, within=within)
    assert np.array_equal(got['marked'] + other['marked'], got['cells'])
    free = run(w, labels, 1, 1, 4, False, values=values, marks=marks, where=where, within=False)
    assert (bits(free['least']) <= bits(got['least'])).all() and ((bits(free['least']) < bits(got['least'])).any() == within)


@pytest.mark.parametrize('L, V, M', list(itertools.product((1, 3), repeat=3)))
@pytest.mark.parametrize('ranked', [True, False])
def test_every_combination_of_store_counts_at_three_fields(L, V, M, ranked):
    w = hand()
    rng = np.random.RandomState(9*L + 3*V + M + ranked)
    labels = w.layer(ranked_labels(rng, 6) if ranked else direct_labels(rng, 6), L)
    values, marks = w.layer(some_values(rng), V), w.layer(some_marks(rng), M)
    got = run(w, labels, L, 3, 6, ranked, values=values, V=V, marks=marks, M=M, within=bool(M & 1))
    if L == 3:
        assert not np.array_equal(got['cells'][:, 0], got['cells'][:, 1])
    else:
        assert np.array_equal(got['cells'][:, 0], got['cells'][:, 2])
        assert np.array_equal(got['marked'][:, 0], got['marked'][:, 1]) == (M == 1)


def test_a_mask_leaves_a_field_as_it_was():
    w = hand()
    rng = np.random.RandomState(4)
    labels, values, marks = w.layer(ranked_labels(rng, 5), 2), w.layer(some_values(rng), 2), w.layer(some_marks(rng), 1)
    mask = rng.rand(w.N, 2) < .5
    mask[1], mask[2] = [True, False], [False, True]
    host = w.host()
    got = host.zones(labels, 2, 2, 4, True, values=values, V=2, marks=marks, mask=mask)
    for key in KEYS:
        assert (got[key][~mask] == -7).all() and (got[key][1, 1] == -7).all(), key
    before = {k: v.copy() for k, v in got.items()}
    want = zone_rule(w.geom, w.starts, CELL, labels, 2, 2, 4, True, values=values, V=2, marks=marks, mask=mask, before=before)
    same(got, want)
    again = host.zones(labels, 2, 2, 4, True, values=values, V=2, marks=marks, mask=~mask, before=got)
    same(again, zone_rule(w.geom, w.starts, CELL, labels, 2, 2, 4, True, values=values, V=2, marks=marks))


def test_direct_labels_below_zero_and_at_k_and_above_are_counted_nowhere():
    w = hand()
    K = 3
    labels = w.layer(lambda n, cells: np.resize(np.array([-1, K, 0, 2, K + 1, -2**31, 2**31 - 1, 2], np.int32), cells), 1)
    got = run(w, labels, 1, 1, K, False, values=w.layer(lambda n, cells: np.ones(cells, F), 1))
    n = 10
    lab = labels[w.at(n):][:w.sizes[n]]
    assert got['cells'][n, 0].tolist() == [int((lab == k).sum()) for k in range(K)] and got['cells'][n, 0, 1] == 0
    assert got['roots'][n, 0].tolist() == [0, -1, 2] and got['n_zones'][n, 0] == 2 and got['nearest'][n, 0].tolist() == [2, -1, 3]


# ---------------------------------------------------------------------------------------------------------------------
# real plans: the regions' and the basins' own outputs as witnesses
# ---------------------------------------------------------------------------------------------------------------------
def _plan_host(w):
    return _ZoneHost(w.geom, w.starts, w.free, cell=w.cell, clearance=w.clearance)


def test_on_the_six_plans_zones_of_the_regions_are_the_regions_own_summary():
    w, _, _, _ = plan_world()
    host = _plan_host(w)
    regions = host.regions()
    K = 256
    assert 1 < regions['counts'].max() <= K
    got = host.zones(regions['labels'], 1, 1, K, True, values=w.values)
    same(got, zone_rule(w.geom, w.starts, w.cell, regions['labels'], 1, 1, K, True, values=w.values))
    assert np.array_equal(got['n_zones'], regions['counts'])
    seeded = 0
    for n in range(w.N):
        at, cells = w.at(n)
        lab = regions['labels'][at:at + cells]
        count = int(regions['counts'][n, 0])
        roots = got['roots'][n, 0, :count]
        assert np.array_equal(roots, np.flatnonzero(lab == np.arange(cells))) and (got['roots'][n, 0, count:] == -1).all()
        assert np.array_equal(got['cells'][n, 0, :count], np.bincount(lab[lab >= 0], minlength=cells)[roots])       # (the label histogram)
        areas = got['cells'][n, 0, :count].astype(F)*(F(w.cell)*F(w.cell))
        assert np.array_equal(bits(areas), bits(regions['areas'][at:at + cells][roots]))
        # the seeded field of two spawn points: 0 in a region that holds a seed, +inf in every other
        holds = np.array([bool((w.values[at:at + cells][lab == r] == 0).any()) for r in roots])
        assert holds.any() and not holds.all()
        assert (got['least'][n, 0, :count][holds] == 0).all() and np.isinf(got['least'][n, 0, :count][~holds]).all()
        assert (w.values[at:at + cells][got['nearest'][n, 0, :count][holds]] == 0).all()
        seeded += int(holds.sum())
    assert seeded >= w.N


def test_with_a_distance_field_the_goals_region_is_at_zero_and_every_other_at_infinity():
    w, _, _, _ = plan_world()
    host = _plan_host(w)
    regions = host.regions()
    values = np.full(int(w.starts[-1]), INF, F)
    goals = {}
    for n in (0, 3):                                                     # (a plan with straight walls, and an oblique one)
        c = w.cases[n]
        at, cells = w.at(n)
        lab = regions['labels'][at:at + cells]
        goal = int(np.flatnonzero(lab == regions['largest'][n, 0])[cells//50])
        i, j = divmod(goal, c.free.shape[1])
        values[at:at + cells] = nav_rule.field(c.free, tuple(c.geom), w.cell, w.centre(n, i, j)).reshape(-1)      # (a centre: its own anchor, leg 0)
        goals[n] = goal
    got = host.zones(regions['labels'], 1, 1, 256, True, values=values)
    same(got, zone_rule(w.geom, w.starts, w.cell, regions['labels'], 1, 1, 256, True, values=values))
    for n, goal in goals.items():
        zone = got['roots'][n, 0].tolist().index(int(regions['largest'][n, 0]))
        assert got['least'][n, 0, zone] == 0 and got['nearest'][n, 0, zone] == goal
        others = np.arange(256) != zone
        assert np.isinf(got['least'][n, 0, others]).all() and (got['nearest'][n, 0, others] == -1).all()
    assert np.isinf(got['least'][[1, 2, 4, 5]]).all()


def test_on_the_six_plans_zones_of_a_basins_store_with_ids_count_the_basins_sizes():
    w, _, ids, _ = plan_world()
    host = _plan_host(w)
    basins = host.basins(w.values, 1, ids, 2)
    got = host.zones(basins['labels'], 1, 1, 2, False, values=w.values)
    same(got, zone_rule(w.geom, w.starts, w.cell, basins['labels'], 1, 1, 2, False, values=w.values))
    assert np.array_equal(got['cells'], basins['sizes']) and (got['cells'] > 100).all()
    assert (got['n_zones'] == 2).all() and (got['roots'] == [0, 1]).all() and (got['least'] == 0).all()
    for n in range(w.N):                                                 # (the nearest cell of territory k is a seed that agent k marked)
        at, _ = w.at(n)
        assert [int(ids[at + v]) for v in got['nearest'][n, 0]] == [0, 1]


# ---------------------------------------------------------------------------------------------------------------------
# Assignments.choose
# ---------------------------------------------------------------------------------------------------------------------
def choose_by_loop(costs):
    """(A,) list: the rule of modules.Assignments.choose for one (A, K) matrix, pair by pair."""
    A, K = costs.shape
    finite = np.isfinite(costs)
    choice, taken = [-1]*A, [False]*K
    for _ in range(A):
        best = None
        for a in range(A):
            for k in range(K):
                if choice[a] < 0 and not taken[k] and finite[a, k] and (best is None or costs[a, k] < costs[best]):
                    best = (a, k)
        if best is None:
            break
        choice[best[0]], taken[best[1]] = best[1], True
    for a in range(A):
        if choice[a] < 0 and finite[a].any():
            choice[a] = int(np.flatnonzero(np.where(finite[a], costs[a], np.inf) == np.where(finite[a], costs[a], np.inf).min())[0])
    return choice


def choose_cases(seed=0):
    """(50, 3, 8) float32: few distinct values, so that ties abound, with +inf (and NaN) entries, rows and columns planted."""
    rng = np.random.RandomState(seed)
    costs = rng.choice(np.array([.5, 1., 1., 2., 2.5, 4., np.inf], F), (50, 3, 8))
    costs[5:15, :, 3:] = np.inf                                          # (fewer reachable zones than agents, or as many)
    costs[10:15, :, 1:] = np.inf
    costs[15:20, 1] = np.inf                                             # (an agent that can walk nowhere)
    costs[20:24] = np.inf
    costs[24:30, :, ::2] = np.inf
    costs[30:34, 0, 0] = np.nan
    costs[34:40] = costs[34:40, :1]                                      # (every agent the same row: the least a takes the best)
    return costs


def test_choose_is_the_greedy_rule_pair_by_pair():
    from megastep_amd import modules
    costs = choose_cases()
    choice, none = modules.Assignments.choose(torch.as_tensor(costs))
    want = np.array([choose_by_loop(c) for c in costs])
    assert choice.dtype == torch.int64 and np.array_equal(choice.numpy(), want) and np.array_equal(none.numpy(), want < 0)
    assert (want < 0).any() and (want >= 0).all(-1).any()
    # distinct zones wherever an env has as many reachable zones as agents; a shared one only after the untaken ran out
    for c, got in zip(costs, want):
        reachable = np.isfinite(c).any(0).sum()
        if np.isfinite(c).all():
            assert len(set(got.tolist())) == min(3, reachable)
    assert modules.Assignments.choose(torch.tensor([[1., 1.], [1., 1.]]))[0].tolist() == [0, 1]      # (ties: the least a, then the least k)
    assert modules.Assignments.choose(torch.tensor([[2., 1.], [3., 1.]]))[0].tolist() == [1, 0]      # (greedy: a walk of 1 + 3, where the optimal assignment walks 2 + 1)
    assert modules.Assignments.choose(torch.tensor([[float('inf'), 1.], [float('inf'), 2.]]))[0].tolist() == [1, 1]      # (step 2: a taken zone)
    one = modules.Assignments.choose(torch.tensor([[[4., float('inf'), 2., 2.]]]))
    assert one[0].tolist() == [[2]] and one[1].tolist() == [[False]]


def test_the_modules_say_what_they_need():
    from types import SimpleNamespace
    from megastep_amd import modules
    from megastep_amd.demo.envs.floorcoverage import FloorCoverage
    with pytest.raises(RuntimeError, match='shared coverage'):
        modules.Assignments(SimpleNamespace(), SimpleNamespace(shared=False))
    for bad in (0, -2):
        with pytest.raises(RuntimeError, match='refresh'):
            modules.Assignments(SimpleNamespace(), SimpleNamespace(shared=True), refresh=bad)
    with pytest.raises(RuntimeError, match="kind must be .*'assign'"):
        FloorCoverage.expert(None, kind='nearest')
    with pytest.raises(RuntimeError, match='shared=True'):
        FloorCoverage.expert(SimpleNamespace(_coverage=SimpleNamespace(shared=False)), 'assign')


# ---------------------------------------------------------------------------------------------------------------------
# header, loader, refusals
# ---------------------------------------------------------------------------------------------------------------------
FIELDS = ('n_fields', 'labels', 'n_labels', 'values', 'n_values', 'marks', 'n_marks', 'where', 'within_marks', 'ranked', 'max_zones', 'mask',
          'cells', 'marked', 'least', 'nearest', 'points', 'roots', 'n_zones')


def test_the_header_declares_the_call_and_the_abi_stays_17():
    from megastep_amd import _lib
    assert 'ms_nav_zones' in declared_symbols(('megastep_hip.h',)) and 'ms_host_nav_zones' in declared_symbols(('megastep_hip_test.h',))
    assert {'ms_nav_zones', 'ms_host_nav_zones'} <= set(_lib.SYMBOLS)
    text = open(os.path.join(ROOT, 'include', 'megastep_hip.h')).read()
    assert int(re.search(r'#define MS_ABI_VERSION (\d+)', text).group(1)) == _lib.ABI_VERSION == 17
    handle = _lib.lib()
    assert hasattr(handle, 'ms_nav_zones') and hasattr(handle, 'ms_host_nav_zones') and handle.ms_abi_version() == 17
    for name in ('DESIGN.md', 'README.md', 'INTEGRATION.md'):
        assert 'ms_nav_zones' in open(os.path.join(ROOT, name)).read(), name
    assert '3.28' in open(os.path.join(ROOT, 'DESIGN.md')).read()


def test_the_mirror_has_the_c_layout():
    import subprocess
    import tempfile
    from megastep_amd import _lib
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "megastep_hip.h"\nint main(){printf("%zu", sizeof(MsNavZones));' +
           ''.join(f'printf(" %zu", offsetof(MsNavZones, {f}));' for f in FIELDS) + '}')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, 't.c'), 'w').write(src)
        subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), os.path.join(d, 't.c'), '-o', os.path.join(d, 't')])
        got = list(map(int, subprocess.check_output([os.path.join(d, 't')]).split()))
    assert [f for f, _ in _lib.MsNavZones._fields_] == list(FIELDS)
    assert got == [ctypes.sizeof(_lib.MsNavZones)] + [getattr(_lib.MsNavZones, f).offset for f in FIELDS]


def test_bad_arguments_are_refused_before_any_launch():
    from megastep_amd import _lib
    h = _lib.lib()
    fake = 64                                       # (never dereferenced: every call below fails its checks first)
    grid = _lib.MsNavGrid(n_envs=2, cell=.125, clearance=.106, geom=fake, starts=fake, max_framed=100, free_cells=fake)
    ref = ctypes.byref
    good = dict(n_fields=3, labels=fake, n_labels=1, values=fake, n_values=3, marks=fake, n_marks=1, where=1, within_marks=0, ranked=1, max_zones=16,
                mask=None, cells=fake, marked=fake, least=fake, nearest=fake, points=fake, roots=fake, n_zones=fake)
    for entry, device in ((h.ms_nav_zones, True), (h.ms_host_nav_zones, False)):
        tail = (None,) if device else ()
        for bad in (dict(n_fields=0), dict(n_fields=-1), dict(labels=None), dict(n_labels=2), dict(n_labels=0), dict(n_values=2), dict(n_values=0),
                    dict(n_marks=2), dict(n_marks=4), dict(where=2), dict(where=-1), dict(within_marks=2), dict(ranked=2), dict(ranked=-1),
                    dict(max_zones=0), dict(max_zones=-1), dict(max_zones=257), dict(cells=None), dict(marked=None), dict(least=None),
                    dict(nearest=None), dict(points=None), dict(roots=None), dict(n_zones=None), dict(labels=66), dict(values=66), dict(cells=66),
                    dict(marked=66), dict(least=66), dict(nearest=66), dict(points=66), dict(roots=66), dict(n_zones=66)):
            s = _lib.MsNavZones(**{**good, **bad})
            assert entry(ref(grid), ref(s), *tail) == -1, bad
        assert entry(None, None, *tail) == -1 and entry(ref(grid), None, *tail) == -1
        s = _lib.MsNavZones(**good)
        assert entry(None, ref(s), *tail) == -1
    # what goes unread may hold anything: the counts and `where` of a layer that is not given
    w = hand()
    labels = w.layer(lambda n, cells: np.zeros(cells, np.int32), 1)
    got = w.host().zones(labels, 1, 1, 2, False, V=7, M=-3, where=True)
    assert got['cells'][:, 0, 0].tolist() == w.sizes


def test_the_python_call_refuses_what_it_cannot_do():
    from megastep_amd import cuda, nav
    grid = _cpu_grid()
    assert cuda.zones is nav.zones and cuda.Zones is nav.Zones and cuda.ZONE_MAX == nav.ZONE_MAX == 256
    new = lambda shape, dtype=torch.int32: torch.zeros(shape, dtype=dtype)
    regions = cuda.Regions(grid, None, 2, True, None, new(256), new(256, torch.float32), *(new((2, 2)) for _ in range(4)))
    fields = cuda.SeededFields(grid, new(256, torch.uint8), 2, True, None, new(256, torch.float32), new((2, 2)))
    with pytest.raises(RuntimeError, match='GPU'):
        cuda.zones(regions)
    with pytest.raises(RuntimeError, match='GPU'):
        regions.zones(values=fields, marks=grid)
    with pytest.raises(RuntimeError, match='GPU'):
        cuda.Basins(fields, None, 0, new(256), None, new((2, 2))).zones()
    with pytest.raises(RuntimeError, match='Regions, a Basins or a cell_layer'):
        cuda.zones(new(256))
    # a labels source that is not int32
    for bad in (cuda.cell_layer(new(256, torch.float32), 2), cuda.cell_layer(new(256, torch.uint8), 2), fields, grid):
        with pytest.raises(RuntimeError, match='int32'):
            cuda.zones(bad if isinstance(bad, cuda.CellLayer) else cuda.cell_layer(bad), ranked=False, grid=grid)
    layer = cuda.cell_layer(new(256), 2)
    for kw in (dict(), dict(ranked=True), dict(grid=grid)):
        with pytest.raises(RuntimeError, match='ranked= .* and grid='):
            cuda.zones(layer, **kw)
    with pytest.raises(RuntimeError, match='GPU'):
        cuda.zones(layer, ranked=False, grid=grid)
    with pytest.raises(RuntimeError, match='contradicts'):
        cuda.zones(regions, ranked=False)
    with pytest.raises(RuntimeError, match='without a `field`'):
        cuda.zones(cuda.cell_layer(new(256), 2, field=new((2, 2))), ranked=True, grid=grid)
    with pytest.raises(RuntimeError, match='entries'):
        cuda.zones(cuda.cell_layer(new(255), 2), ranked=True, grid=grid)
    # store counts that are neither 1 nor F
    three = cuda.SeededFields(grid, new(384, torch.uint8), 3, True, None, new(384, torch.float32), new((2, 3)))
    for kw in (dict(values=three), dict(marks=cuda.cell_layer(new(384, torch.uint8), 3)), dict(values=fields, marks=cuda.cell_layer(new(384, torch.uint8), 3))):
        with pytest.raises(RuntimeError, match='must have 1 or F = 3'):
            cuda.zones(regions, **kw)
    with pytest.raises(RuntimeError, match='float32'):
        cuda.zones(regions, values=grid)
    with pytest.raises(RuntimeError, match='uint8'):
        cuda.zones(regions, marks=fields)
    with pytest.raises(RuntimeError, match='labels'):
        cuda.zones(regions, values=layer)
    for bad in (0, -1, 257, 1.5, True):
        with pytest.raises(RuntimeError, match='n_zones'):
            cuda.zones(regions, n_zones=bad)
    # a wrong `out`
    z = cuda.Zones(grid, regions, regions.labels, 2, fields.values, 2, None, 1, True, False, True, 2, 16, lambda shape, dtype, fill: torch.full(shape, fill, dtype=dtype))
    assert z.cells.shape == (2, 2, 16) and z.points.shape == (2, 2, 16, 2) and z.n_zones.shape == (2, 2) and z.areas().shape == (2, 2, 16)
    other = cuda.Regions(grid, None, 2, True, None, new(256), new(256, torch.float32), *(new((2, 2)) for _ in range(4)))
    for source, kw in ((other, {}), (regions, dict(values=None)), (regions, dict(n_zones=8)), (regions, dict(marks=grid)), (regions, dict(where=False)),
                       (regions, dict(within_marks=True))):
        with pytest.raises(RuntimeError, match='`out` must come from a zones call'):
            cuda.zones(source, **{**dict(values=fields, n_zones=16), **kw}, out=z)
    with pytest.raises(RuntimeError, match='`out` must come from a zones call'):
        cuda.zones(regions, values=fields, out=regions)
    for bad in (torch.ones((2, 2)), torch.ones((2, 3), dtype=torch.bool)):
        with pytest.raises(RuntimeError, match='mask'):
            z.update(bad)
    with pytest.raises(RuntimeError, match='GPU'):
        cuda.zones(regions, values=fields, out=z)
    # the layers the other calls take do not take labels
    with pytest.raises(RuntimeError, match='only zones'):
        cuda.map_channel(layer)
