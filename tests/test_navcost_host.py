"""Cost fields (`ms_nav_cost_fields` / `ms_nav_cost_waypoints` / `ms_nav_cost_paths`, `cuda.cost_fields`, `cuda.inflation_costs`,
`cuda.mark_costs`, `modules.Routes`) on the CPU: the contract of include/megastep_hip.h (MsNavCostFields) restated in binary32
numpy (`cost_rule`, which tests/test_gpu_navcost.py holds the kernels to, bit for bit); the freedom of schedule it rests on; the
host instantiations of the kernels' own per-cell functions against the rule; the reduction to the seeded fields, the clamp, the
bounds the weights imply; the followers and a walker; and the C-ABI's declarations, layouts and refusals."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests.test_abi import ROOT, declared_symbols
from tests.test_navfield_host import CELL, CELLS, DIAGONAL, RADIUS, F, INF, _crossings, _distance_to_walls, bits, nav_rule
from tests.test_navpath_host import NEIGHBOURS, path_rule
from tests.test_navseed_host import _SPARE, cases, host_field, seed_rule

COST_MAX = F(256)


class cost_rule:
    """The contract in numpy: seed_rule with a multiplier per cell and the weights of the cell a step leaves; every operation one
    binary32 operation, in the order the header gives. `cost` is (ny, nx) float32."""

    @staticmethod
    def multiplier(x):
        """k = x >= 1.f ? fminf(x, 256.f) : (x < 1.f ? 1.f : 256.f): below 1 is 1, above 256 is 256, a NaN is 256."""
        x = np.asarray(x, F)
        with np.errstate(invalid='ignore'):
            return np.where(x >= 1, np.fmin(x, COST_MAX), np.where(x < 1, F(1), COST_MAX)).astype(F)

    @staticmethod
    def weights(cell, k):
        """(ws, wd) = (fl(c k), fl(fl(c 1.41421356f) k))."""
        k = np.asarray(k, F)
        return (F(cell)*k).astype(F), ((F(cell)*DIAGONAL)*k).astype(F)

    @staticmethod
    def edges(free, cell, cost):
        """(u, v, w): nav_rule's directed edges u -> v (D[v] is lowered from D[u]); the hop towards the seeds leaves v, so the
        weight is v's."""
        u, v, w = nav_rule.edges(free, cell)
        ws, wd = cost_rule.weights(cell, cost_rule.multiplier(cost).reshape(-1))
        nx = free.shape[1]
        straight = (u // nx == v // nx) | (u % nx == v % nx)
        return u, v, np.where(straight, ws[v], wd[v]).astype(F)

    @staticmethod
    def graph(free, cell, cost):
        u, v, w = cost_rule.edges(free, cell, cost)
        order = np.argsort(u, kind='stable')
        u, v, w = u[order], v[order], w[order]
        return np.searchsorted(u, np.arange(free.size + 1)), v, w

    @staticmethod
    def field(free, cell, seeds, cost):
        """The field by a multi-source heap Dijkstra with binary32 additions over the weighted edges."""
        return seed_rule.field(free, cell, seeds, cost_rule.graph(free, cell, cost))

    @staticmethod
    def field_by_sweeps(free, cell, seeds, cost):
        u, v, w = cost_rule.edges(free, cell, cost)
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
    def field_by_random_order(free, cell, seeds, cost, seed, chunks=6):
        u, v, w = cost_rule.edges(free, cell, cost)
        rng = np.random.RandomState(seed)
        D = np.where(seeds.reshape(-1), F(0), INF).astype(F)
        while True:
            before = D.copy()
            for part in np.array_split(rng.permutation(len(u)), chunks):
                np.minimum.at(D, v[part], D[u[part]] + w[part])
            if np.array_equal(before, D):
                return D.reshape(free.shape)

    @staticmethod
    def hops(world, cost):
        """seed_rule's hop table with the weights of the cell the hop leaves: (kind, step, least)."""
        geom, cell, free, D = world
        ny, nx = D.shape
        ws, wd = cost_rule.weights(cell, cost_rule.multiplier(cost))
        pf = np.zeros((ny + 2, nx + 2), bool); pf[1:-1, 1:-1] = free
        pd = np.full((ny + 2, nx + 2), INF, F); pd[1:-1, 1:-1] = D
        best, below = np.full((ny, nx), INF, F), np.full((ny, nx), INF, F)
        step = np.full((ny, nx), -1, np.int8)
        for t, (di, dj) in enumerate(NEIGHBOURS):
            ok = pf[1 + di:ny + 1 + di, 1 + dj:nx + 1 + dj]
            if di and dj:
                ok = ok & pf[1 + di:ny + 1 + di, 1:nx + 1] & pf[1:ny + 1, 1 + dj:nx + 1 + dj]
            du = pd[1 + di:ny + 1 + di, 1 + dj:nx + 1 + dj]
            with np.errstate(all='ignore'):
                v = np.where(ok, du + (wd if di and dj else ws), INF)
                take = v < best
            best, below, step = np.where(take, v, best), np.where(take, du, below), np.where(take, np.int8(t), step)
        with np.errstate(all='ignore'):
            kind = np.where((step >= 0) & (below < D), 1, -1).astype(np.int8)
            kind[D == 0] = 0
        return kind, step, best

    waypoint = staticmethod(seed_rule.waypoint)      # (with cost_rule.hops' table)
    path = staticmethod(seed_rule.path)
    chain = staticmethod(seed_rule.chain)
    query = staticmethod(seed_rule.query)


# ---------------------------------------------------------------------------------------------------------------------
# the cost layers' formulas in numpy, and the host instantiations
# ---------------------------------------------------------------------------------------------------------------------
def inflation(d, radius, weight=4.):
    """cuda.inflation_costs: 1 + weight*clamp(1 - d/radius, 0, 1), binary32."""
    d = np.asarray(d, F)
    with np.errstate(invalid='ignore'):
        return (np.clip(F(1) - d/F(radius), F(0), F(1))*F(weight) + F(1)).astype(F)


def marked(layer, on=1., off=256., where=True):
    """cuda.mark_costs without a gate."""
    return np.where((np.asarray(layer) != 0) == bool(where), F(on), F(off)).astype(F)


def clearance_of(case):
    """(ny, nx) float32: the distance from every cell's centre to the nearest wall (float64, rounded: an input, not a rule)."""
    x, y = nav_rule.centres(case.geom, case.cell)
    pts = np.stack(np.broadcast_arrays(x[None, :], y[:, None]), -1).reshape(-1, 2)
    return _distance_to_walls(pts, case.walls).astype(F).reshape(case.free.shape)


def host_cost_field(geom, cell, free, marks, where, among, cost, framed=0):
    """ms_host_nav_cost_field: (D (ny, nx), n_seeds, sweeps)."""
    from megastep_amd import _lib
    h = _lib.lib()
    geom = np.array(geom, np.int32)
    free, marks = np.ascontiguousarray(free, np.uint8), np.ascontiguousarray(marks, np.uint8)
    among = None if among is None else np.ascontiguousarray(among, np.uint8)
    cost = None if cost is None else np.ascontiguousarray(cost, F)
    D = np.full(free.shape, -7., F)
    n = ctypes.c_int(-7)
    ptr = lambda a: None if a is None else (a.ctypes.data or _SPARE.ctypes.data)
    sweeps = h.ms_host_nav_cost_field(ptr(geom), cell, ptr(free), ptr(marks), int(where), ptr(among), ptr(cost), framed, ptr(D), ctypes.addressof(n))
    return D, n.value, sweeps


def host_cost_follow(world, cost, p, lookahead=None, max_points=None):
    from megastep_amd import _lib
    geom, cell, free, D = world
    h = _lib.lib()
    geom = np.array(geom, np.int32)
    free, D, p, cost = np.ascontiguousarray(free, np.uint8), np.ascontiguousarray(D, F), np.ascontiguousarray(p, F), np.ascontiguousarray(cost, F)
    ptr = lambda a: a.ctypes.data or _SPARE.ctypes.data
    if lookahead is not None:
        out = np.zeros(2, F)
        k = h.ms_host_nav_cost_waypoint(ptr(geom), cell, ptr(free), ptr(D), ptr(cost), ptr(p), lookahead, ptr(out))
        return out, k
    out = np.zeros((max_points, 2), F)
    count = h.ms_host_nav_cost_path(ptr(geom), cell, ptr(free), ptr(D), ptr(cost), ptr(p), max_points, ptr(out))
    return out, count


def _same(world, cost, p, table, lookaheads=(16,), max_points=(8,)):
    for L in lookaheads:
        got, k = host_cost_follow(world, cost, p, lookahead=L)
        want, wk = cost_rule.waypoint(world, p, L, table)
        assert k == wk and bits(got).tolist() == bits(np.array(want, F)).tolist(), (p, L, k, wk)
    for M in max_points:
        got, count = host_cost_follow(world, cost, p, max_points=M)
        want, wcount = cost_rule.path(world, p, M, table)
        assert count == wcount and np.array_equal(bits(got), bits(want)), (p, M, count, wcount)
    return wk, wcount


# ---------------------------------------------------------------------------------------------------------------------
# the inputs: the seeded suite's plans and seed sets (three plain and three oblique plans, the floor a ring of rays has not seen
# and the floor it has), each under two cost layers - an inflation layer of radius 0.5 m, which an env's fields share (one store
# an env), and a known-space layer over the case's own seen map (one store a field)
# ---------------------------------------------------------------------------------------------------------------------
INFLATION_RADIUS = .5


class _Costed:
    """A seeded case under one cost layer: its field by the rule and its hop table."""

    def __init__(self, case, cost, kind):
        self.case, self.cost, self.kind = case, np.ascontiguousarray(cost, F), kind
        self.D = cost_rule.field(case.free, case.cell, case.seeds, self.cost)
        self.world = (case.geom, case.cell, case.free, self.D)
        self.table = cost_rule.hops(self.world, self.cost)


_COSTED, _CLEAR = {}, {}


def inflation_of(case):
    key = (case.cell, id(case.walls))
    if key not in _CLEAR:
        _CLEAR[key] = inflation(clearance_of(case), INFLATION_RADIUS)
    return _CLEAR[key]


def costed(cell=CELL, r=RADIUS, kinds=('inflation', 'known')):
    found = []
    for k, case in enumerate(cases(cell, r)):
        for kind in kinds:
            key = (cell, r, k, kind)
            if key not in _COSTED:
                _COSTED[key] = _Costed(case, inflation_of(case) if kind == 'inflation' else marked(case.marks), kind)
            found.append(_COSTED[key])
    return found


def worth_comparing(found):
    """The conditions that keep the equalities from being vacuous, by the numpy rule alone.  Of a list of costed cases, those whose
    field has at least one seed and is finite on at least half of its free cells: most of the list, every plan among them.  And of
    the cells the inflated fields are compared on - finite under both weights - at least a quarter differ from the unweighted
    field's, or the comparison would pass on a kernel that ignores the costs."""
    good = [c for c in found if c.case.seeds.any() and np.isfinite(c.D).sum() >= .5*c.case.free.sum()]
    assert len(good) >= .75*len(found) and len({id(c.case.walls) for c in good}) == len({id(c.case.walls) for c in found})
    inflated = [c for c in good if c.kind == 'inflation']
    assert inflated
    differ = total = 0
    for c in inflated:
        both = np.isfinite(c.D) & np.isfinite(c.case.D)
        differ += int((bits(c.D)[both] != bits(c.case.D)[both]).sum())
        total += int(both.sum())
    assert differ >= .25*total and total > 500*len(inflated), (differ, total)
    return good


def test_the_inputs_are_worth_comparing():
    good = worth_comparing(costed())
    assert all(c.case.seeds.any() and np.isfinite(c.D).sum() >= .5*c.case.free.sum() for c in good)
    # the layers are no constants: an inflation layer spans [1, 1 + weight) on the free cells, a known-space one has both prices
    for c in good:
        on_free = c.cost[c.case.free]
        assert on_free.min() == 1 and (on_free.max() > 3 if c.kind == 'inflation' else on_free.max() == 256)


# ---------------------------------------------------------------------------------------------------------------------
# the rule itself
# ---------------------------------------------------------------------------------------------------------------------
def test_the_multiplier_on_hand_values():
    x = np.array([0, -3, -np.inf, 1e-40, .999, 1, 1.5, 255.5, 256, 257, 1e30, np.inf, np.nan, -np.nan], F)
    want = np.array([1, 1, 1, 1, 1, 1, 1.5, 255.5, 256, 256, 256, 256, 256, 256], F)
    assert np.array_equal(bits(cost_rule.multiplier(x)), bits(want))
    ws, wd = cost_rule.weights(.1, np.array([1, 3], F))
    assert bits(ws[0]) == bits(F(.1)) and bits(wd[0]) == bits(F(.1)*DIAGONAL)              # (times 1.f is exact)
    assert bits(wd[1]) == bits((F(.1)*DIAGONAL)*F(3)) and bits(wd[1]) != bits(F(.1)*(DIAGONAL*F(3)))        # (the order matters)


def test_any_schedule_ends_on_the_same_bits():
    """Multi-source Dijkstra, synchronous sweeps and a seeded random order of the weighted edges: equal as uint32, infinities
    included."""
    for k, c in enumerate(worth_comparing(costed())[::3]):
        case = c.case
        swept, sweeps = cost_rule.field_by_sweeps(case.free, case.cell, case.seeds, c.cost)
        shuffled = cost_rule.field_by_random_order(case.free, case.cell, case.seeds, c.cost, seed=k)
        assert sweeps > 5
        assert np.array_equal(bits(c.D), bits(swept))
        assert np.array_equal(bits(c.D), bits(shuffled))
        assert np.isinf(c.D[~case.free]).all() and np.array_equal(c.D == 0, case.seeds)


# ---------------------------------------------------------------------------------------------------------------------
# the kernels' own per-cell functions, instantiated on the host
# ---------------------------------------------------------------------------------------------------------------------
def _host_field_is_the_rule(found):
    for c in found:
        case = c.case
        for framed in (0, 1):
            D, n, sweeps = host_cost_field(case.geom, case.cell, case.free, case.marks, case.where, case.among, c.cost, framed)
            assert n == case.seeds.sum() and sweeps >= 2
            assert np.array_equal(bits(D), bits(c.D)), (c.kind, framed, int((bits(D) != bits(c.D)).sum()))


def test_the_host_field_is_the_rule_bit_for_bit():
    """On the six plans, both seed sets, a cost store an env shares (inflation) and one of the field's own (known space)."""
    _host_field_is_the_rule(worth_comparing(costed()))


@pytest.mark.parametrize('cell,r', CELLS)
def test_the_host_field_is_the_rule_at_other_cell_widths(cell, r):
    _host_field_is_the_rule(worth_comparing(costed(cell, r)))


def _hand_made():
    """[(name, free, marks, cost)]: small grids whose fields can be worked out by hand or that sit on an edge of the rule."""
    rng = np.random.RandomState(12)
    out = []
    free = np.ones((1, 1), bool); out.append(('one cell, a seed', free, np.ones((1, 1), np.uint8), np.full((1, 1), 9, F)))
    free = np.ones((1, 9), bool); m = np.zeros((1, 9), np.uint8); m[0, 0] = 1
    out.append(('a row', free, m, np.arange(1, 10, dtype=F).reshape(1, 9)))
    free = np.ones((9, 1), bool); m = np.zeros((9, 1), np.uint8); m[8, 0] = 1
    out.append(('a column', free, m, np.linspace(.5, 300, 9).astype(F).reshape(9, 1)))
    free = np.ones((7, 11), bool); m = np.zeros((7, 11), np.uint8); m[3, 0] = 1
    cost = np.ones((7, 11), F); cost[1:6, 5] = 40                      # a dear bar with cheap gaps at both ends
    out.append(('a bar to walk round', free, m, cost))
    free = np.ones((8, 8), bool); free[2:6, 3] = False; free[5, 3:7] = False
    m = np.zeros((8, 8), np.uint8); m[0, 0] = m[7, 7] = 1
    out.append(('walls and corners under a gradient', free, m, (1 + np.add.outer(np.arange(8), np.arange(8))*.37).astype(F)))
    free = rng.rand(13, 17) > .25; m = (rng.rand(13, 17) < .03).astype(np.uint8)
    out.append(('noise', free, m, np.exp(rng.uniform(-1, 7, (13, 17))).astype(F)))
    cost = np.full((6, 6), 256, F); m = np.zeros((6, 6), np.uint8); m[5, 5] = 1
    out.append(('the dearest everywhere', np.ones((6, 6), bool), m, cost))
    out.append(('every free cell a seed', free, np.ones((13, 17), np.uint8), np.full((13, 17), 7, F)))
    out.append(('no seed', free, np.zeros((13, 17), np.uint8), np.full((13, 17), 7, F)))
    return out


def test_hand_made_grids():
    for name, free, marks, cost in _hand_made():
        geom = (-3, 2, free.shape[1], free.shape[0])
        seeds = seed_rule.seeds(free, marks, 1)
        want = cost_rule.field(free, .1, seeds, cost)
        for framed in (0, 1):
            D, n, _ = host_cost_field(geom, .1, free, marks, 1, None, cost, framed)
            assert n == seeds.sum() and np.array_equal(bits(D), bits(want)), (name, framed)
    # known answers.  A row from its left end: cell j is left j times, each step at the cost of the cell left
    _, free, marks, cost = _hand_made()[1]
    D = cost_rule.field(free, .1, marks == 1, cost)[0]
    acc = [F(0)]
    for j in range(1, 9):
        acc.append(F(acc[-1] + F(.1)*cost[0, j]))
    assert np.array_equal(bits(D), bits(np.array(acc, F)))
    # the seed's own cost is never charged, the far end's is
    assert D[1] == F(.1)*F(2) and D[0] == 0
    # the bar: the cheapest way from the far side goes round the bar's end, not through it
    _, free, marks, cost = _hand_made()[3]
    D = cost_rule.field(free, .1, marks == 1, cost)
    flat = seed_rule.field(free, .1, marks == 1)
    assert D[3, 10] > flat[3, 10] and D[3, 10] < flat[3, 10] + F(.1)*F(8)        # a detour of a few cells, not a step of 40
    kind, step, _ = cost_rule.hops(((0, 0, 11, 7), .1, free, D), cost)
    i, j, crossed = 3, 10, []
    while kind[i, j] == 1:
        crossed.append(cost[i, j])
        i, j = i + NEIGHBOURS[step[i, j]][0], j + NEIGHBOURS[step[i, j]][1]
    assert kind[i, j] == 0 and max(crossed) == 1


def test_a_cost_of_one_and_costs_below_one_give_the_seeded_fields_bits():
    """The reduction: all 1.f, and any values <= 1 (0, -3, -inf, subnormals), give ms_host_nav_seed_field's bits - and the rule's."""
    rng = np.random.RandomState(2)
    for case in cases()[::2] + cases(*CELLS[1])[::4]:
        seeded = [host_field(case.geom, case.cell, case.free, case.marks, case.where, case.among, framed)[0] for framed in (0, 1)]
        assert np.array_equal(bits(seeded[0]), bits(case.D)) and np.array_equal(bits(seeded[1]), bits(case.D))
        low = rng.choice(np.array([0, -0., -3, -np.inf, 1e-40, -1e-45, .5, 1, np.nextafter(F(1), F(0))], F), case.free.shape)
        for cost in (np.ones(case.free.shape, F), low):
            assert np.array_equal(bits(cost_rule.field(case.free, case.cell, case.seeds, cost)), bits(case.D))
            for framed in (0, 1):
                D, n, _ = host_cost_field(case.geom, case.cell, case.free, case.marks, case.where, case.among, cost, framed)
                assert n == case.seeds.sum() and np.array_equal(bits(D), bits(seeded[framed]))


def clamp_layers(shape, rng):
    """(odd, tame): a layer salted with +inf, 1e30 and NaNs, and the layer holding 256.f there."""
    tame = np.exp(rng.uniform(0, 3, shape)).astype(F)
    odd = tame.copy()
    salt = rng.rand(*shape)
    odd[salt < .1] = np.inf
    odd[(salt >= .1) & (salt < .2)] = 1e30
    odd[(salt >= .2) & (salt < .3)] = np.nan
    odd[(salt >= .3) & (salt < .35)] = 257
    tame[salt < .35] = 256
    return odd, tame


def test_costs_beyond_the_clamp_and_nans_count_as_256():
    rng = np.random.RandomState(4)
    for case in cases()[::3]:
        odd, tame = clamp_layers(case.free.shape, rng)
        want = cost_rule.field(case.free, case.cell, case.seeds, tame)
        assert np.array_equal(bits(cost_rule.field(case.free, case.cell, case.seeds, odd)), bits(want))
        for framed in (0, 1):
            for cost in (odd, tame):
                D, _, _ = host_cost_field(case.geom, case.cell, case.free, case.marks, case.where, case.among, cost, framed)
                assert np.array_equal(bits(D), bits(want))
        # ... and a NaN is the dearest, not the cheapest: the field of a layer of NaNs is the field at 256 throughout
        D, _, _ = host_cost_field(case.geom, case.cell, case.free, case.marks, case.where, case.among, np.full(case.free.shape, np.nan, F))
        assert np.array_equal(bits(D), bits(cost_rule.field(case.free, case.cell, case.seeds, np.full(case.free.shape, 256, F))))


def test_a_cost_field_is_never_below_the_seeded_one_and_finite_on_the_same_cells():
    for c in worth_comparing(costed()):
        assert np.array_equal(np.isfinite(c.D), np.isfinite(c.case.D))   # (no cost closes a cell)
        assert (c.D >= c.case.D).all()


def test_no_path_is_cheaper_than_the_field_says():
    """Optimality: for a start, the path the UNWEIGHTED follower takes, priced under the cost's weights - the left-to-right
    binary32 sum from the seed outward, each step at the weights of the cell it leaves - is at least D_cost[start]."""
    checked = dearer = 0
    for c in worth_comparing(costed()):
        case = c.case
        ws, wd = cost_rule.weights(case.cell, cost_rule.multiplier(c.cost))
        for p in case.points[::5]:
            found = seed_rule.chain(case.world, p, None, case.table)
            if found is None or not found[1]:
                continue
            cells = found[3]
            total = F(0)
            for (i, j), (ni, nj) in zip(cells[-2::-1], cells[:0:-1]):   # the step out of (i, j) into (ni, nj), last step first
                total = F(total + (wd[i, j] if ni != i and nj != j else ws[i, j]))
            assert total >= c.D[cells[0]], (p, total, c.D[cells[0]])
            checked += 1
            dearer += total > c.D[cells[0]]
    assert checked > 500 and dearer > 100


# ---------------------------------------------------------------------------------------------------------------------
# the followers
# ---------------------------------------------------------------------------------------------------------------------
def _host_followers_are_the_rule(found, stride):
    finite = total = cut = 0
    for c in found:
        case = c.case
        for k, p in enumerate(case.points[::stride]):
            many = k % 16 == 0
            hops, count = _same(c.world, c.cost, p, c.table, (1, 2, 16, 64) if many else (16,), (8, 256) if many else (8,))
            total += 1
            finite += hops >= 0
            cut += count > 8
            assert (hops < 0) == (count == 0) == bool(np.isinf(cost_rule.query(c.world, p)))
            assert count >= 0                                            # (a settled field never breaks a chain)
        lo, hi = case.walls.reshape(-1, 2).min(0), case.walls.reshape(-1, 2).max(0)
        rng = np.random.RandomState(5)
        odd = list(lo - .3 + rng.uniform(0, 1, (20, 2))*(hi - lo + .6)) + [lo - 5., hi + 1e6, [np.nan, 2.], [2., np.inf], [-3e38, 3e38]]
        none = sum(_same(c.world, c.cost, np.array(p, F), c.table, (1, 16, 64))[1] == 0 for p in odd)
        assert 5 <= none < len(odd)
    assert finite >= .8*total and cut > 100/stride, (finite, total, cut)


def test_the_host_followers_are_the_rule_bit_for_bit():
    _host_followers_are_the_rule(worth_comparing(costed()), 4)


@pytest.mark.parametrize('cell,r', CELLS)
def test_the_host_followers_are_the_rule_at_other_cell_widths(cell, r):
    _host_followers_are_the_rule(worth_comparing(costed(cell, r)), 12)


def test_on_a_settled_field_no_chain_breaks_from_any_finite_cell():
    """Every cell with a finite value hops to a strictly lower neighbour or is a seed, and the chain from it ends on a seed."""
    for c in worth_comparing(costed()):
        kind, step, least = c.table
        finite = np.isfinite(c.D)
        assert (kind[finite] >= 0).all() and np.array_equal(kind == 0, c.case.seeds)
        on = finite & (kind == 1)
        assert np.array_equal(bits(least[on]), bits(c.D[on]))           # (at the fixed point the least neighbour value IS D[v])
        x, y = nav_rule.centres(c.case.geom, c.case.cell)
        cells = np.argwhere(finite)[::37]
        for i, j in cells:
            pts, count = host_cost_follow(c.world, c.cost, (x[j], y[i]), max_points=4)
            assert count >= 2


def test_the_hop_follows_the_weighted_field_where_the_unweighted_hop_would_not():
    """What the weights of the hop are for: on the inflated fields some cell's unweighted hop (the least D[u] + plain w) names
    another neighbour than the weighted one does, and the paths differ."""
    other = 0
    for c in worth_comparing(costed())[:4]:
        if c.kind != 'inflation':
            continue
        plain = seed_rule.hops(c.world)
        on = np.isfinite(c.D) & (c.table[0] == 1)
        other += int((plain[1][on] != c.table[1][on]).sum())
    assert other > 50


def test_a_stale_or_garbage_field_breaks_the_chain_and_nothing_hangs():
    c = worth_comparing(costed())[0]
    a = c.case
    flat = (a.geom, a.cell, a.free, np.full_like(c.D, 3.))
    table = cost_rule.hops(flat, c.cost)
    counts = [_same(flat, c.cost, p, table, (1, 16), (8,))[1] for p in a.points[:20]]
    assert set(counts) <= {-2, 0} and counts.count(-2) >= 16
    rng = np.random.RandomState(3)
    D = c.D.copy()
    D[rng.rand(*D.shape) < .05] = np.nan
    D[rng.rand(*D.shape) < .05] = -np.inf
    D[rng.rand(*D.shape) < .05] = -2.
    D[rng.rand(*D.shape) < .02] = 0.
    junk = (a.geom, a.cell, a.free, D)
    odd, _ = clamp_layers(D.shape, rng)
    for cost in (c.cost, odd):
        table = cost_rule.hops(junk, cost)
        for p in a.points[:40]:
            _same(junk, cost, p, table, (16, 64), (8, 64))
    # the seeded field followed with weights it was not made with: stale - chains may break, each returns
    table = cost_rule.hops(a.world, c.cost)
    for p in a.points[:40]:
        _same(a.world, c.cost, p, table, (16,), (64,))


def test_a_walker_that_follows_the_waypoints_of_an_inflated_field_reaches_a_seed():
    """A point walker taking 0.1 m steps towards its current waypoint: from every start with a path it ends on the centre of a
    cell at 0, and no segment to a waypoint meets a wall."""
    rng = np.random.RandomState(9)
    walks = 0
    for c in worth_comparing(costed(kinds=('inflation',))):
        case = c.case
        starts, ends = [], []
        for p0 in case.points[rng.choice(len(case.points), 24, replace=False)]:
            if not np.isfinite(cost_rule.query(c.world, p0)):
                continue
            p, arrived = p0.copy(), False
            for _ in range(3000):
                w, k = cost_rule.waypoint(c.world, p, 16, c.table)
                assert k >= 0
                w = np.array(w, F)
                starts.append(p.copy()); ends.append(w)
                d = np.linalg.norm(w.astype(np.float64) - p)
                if d <= .1:
                    p = w
                    i, j = path_rule.corner(p + F(case.cell/2), case.geom, case.cell)
                    if c.D[i, j] == 0 and bits(np.array(path_rule.centre(case.geom, case.cell, i, j), F)).tolist() == bits(p).tolist():
                        arrived = True
                        break
                else:
                    p = (p + (w.astype(np.float64) - p)*(.1/d)).astype(F)
            assert arrived, (p0, p)
            walks += 1
        assert _crossings(np.array(starts), np.array(ends), case.walls) == 0
    assert walks > 100


def test_an_inflated_path_keeps_further_from_the_walls():
    """What the layer is for, on the rule alone: over the starts of the inflated cases the cells of the weighted path are, in the
    mean, further from the nearest wall than the cells of the unweighted one."""
    gain = []
    for c in worth_comparing(costed(kinds=('inflation',))):
        clear = clearance_of(c.case)
        for p in c.case.points[::9]:
            a, b = seed_rule.chain(c.case.world, p, None, c.case.table), cost_rule.chain(c.world, p, None, c.table)
            if a is None or len(a[3]) < 8:
                continue
            gain.append(np.mean([clear[v] for v in b[3]]) - np.mean([clear[v] for v in a[3]]))
    assert len(gain) > 200 and np.mean(gain) > .02 and np.mean(np.array(gain) >= 0) > .7, (len(gain), np.mean(gain))


# ---------------------------------------------------------------------------------------------------------------------
# header, loader, refusals
# ---------------------------------------------------------------------------------------------------------------------
COST_SYMBOLS = {'ms_nav_cost_fields', 'ms_nav_cost_waypoints', 'ms_nav_cost_paths'}
HOST_SYMBOLS = {'ms_host_nav_cost_field', 'ms_host_nav_cost_waypoint', 'ms_host_nav_cost_path', 'ms_host_nav_cost_capacity',
                'ms_debug_nav_cost_variant'}


def test_the_cost_capacities_are_the_librarys():
    """cuda.COST_CAPACITY is what the instantiations that keep the multipliers in LDS hold, in framed cells: two floats and a byte
    a cell in 40, 80 and 160 KiB less the flags, a multiple of four."""
    from megastep_amd import _lib, cuda, nav
    caps = (ctypes.c_int*3)()
    assert _lib.lib().ms_host_nav_cost_capacity(caps) == 0 and tuple(caps) == nav.COST_CAPACITY == (4544, 9092, 18196)
    assert tuple(caps) == tuple((kib*1024 - 64)//9//4*4 for kib in (40, 80, 160))
    assert _lib.lib().ms_host_nav_cost_capacity(None) == -1
    assert cuda.COST_CAPACITY is nav.COST_CAPACITY and cuda.COST_MAX == nav.COST_MAX == 256.
    assert all(9*c + 16 <= kib*1024 for c, kib in zip(caps, (40, 80, 160)))
    h = _lib.lib()
    assert [h.ms_debug_nav_cost_variant(v) for v in (0, 1, -1)] == [0, 0, 0]
    assert h.ms_debug_nav_cost_variant(2) == -1 and h.ms_debug_nav_cost_variant(-2) == -1


def test_the_header_declares_the_cost_calls_and_the_loader_binds_them():
    from megastep_amd import _lib
    assert COST_SYMBOLS <= set(declared_symbols(('megastep_hip.h',)))
    assert HOST_SYMBOLS <= set(declared_symbols(('megastep_hip_test.h',)))
    assert COST_SYMBOLS | HOST_SYMBOLS <= set(_lib.SYMBOLS)
    text = open(os.path.join(ROOT, 'include', 'megastep_hip.h')).read()
    assert int(re.search(r'#define MS_ABI_VERSION (\d+)', text).group(1)) == _lib.ABI_VERSION == 17
    handle = _lib.lib()
    assert all(hasattr(handle, s) for s in COST_SYMBOLS | HOST_SYMBOLS) and handle.ms_abi_version() == 17


@pytest.mark.parametrize('name,fields', [
    ('MsNavCostFields', ('n_fields', 'marks', 'where', 'among', 'mask', 'fields', 'passes', 'n_seeds', 'costs', 'n_costs')),
    ('MsNavCostWaypoints', ('n_points', 'points', 'goal', 'fields', 'n_goals', 'lookahead', 'waypoints', 'hops', 'costs', 'n_costs')),
    ('MsNavCostPaths', ('n_points', 'points', 'goal', 'fields', 'n_goals', 'max_points', 'paths', 'counts', 'costs', 'n_costs'))])
def test_the_cost_mirrors_have_the_c_layout(name, fields):
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


def test_bad_cost_arguments_are_refused_before_any_launch():
    from megastep_amd import _lib
    h = _lib.lib()
    fake = 64                                       # (never dereferenced: every call below fails its checks first)
    grid = dict(n_envs=2, cell=.125, clearance=.106, geom=fake, starts=fake, max_framed=100, free_cells=fake)
    seed = dict(n_fields=3, marks=fake, where=0, among=None, mask=None, fields=fake, passes=None, n_seeds=None, costs=fake, n_costs=3)
    way = dict(n_points=3, points=fake, goal=None, fields=fake, n_goals=3, lookahead=16, waypoints=fake, hops=None, costs=fake, n_costs=1)
    path = dict(n_points=3, points=fake, goal=None, fields=fake, n_goals=3, max_points=8, paths=fake, counts=fake, costs=fake, n_costs=3)
    G, S, W, P = _lib.MsNavGrid, _lib.MsNavCostFields, _lib.MsNavCostWaypoints, _lib.MsNavCostPaths
    ref = ctypes.byref
    calls = ((h.ms_nav_cost_fields, S, seed), (h.ms_nav_cost_waypoints, W, way), (h.ms_nav_cost_paths, P, path))
    for call, kind, good in calls:
        assert call(None, ref(kind(**good)), None) == -1
        assert call(ref(G(**grid)), None, None) == -1
        for bad in (dict(n_envs=0), dict(cell=0.), dict(cell=float('nan')), dict(clearance=0.), dict(cell=.15), dict(geom=None),
                    dict(starts=None), dict(free_cells=None), dict(max_framed=-1), dict(geom=68)):
            assert call(ref(G(**{**grid, **bad})), ref(kind(**good)), None) == -1, bad
        for bad in (dict(costs=None), dict(costs=66), dict(n_costs=0), dict(n_costs=2), dict(n_costs=4), dict(n_costs=-1)):
            assert call(ref(G(**grid)), ref(kind(**{**good, **bad})), None) == -1, bad
    for bad in (dict(n_fields=0), dict(n_fields=-2), dict(marks=None), dict(fields=None), dict(where=2), dict(where=-1), dict(where=256),
                dict(fields=66), dict(passes=66), dict(n_seeds=66)):
        assert h.ms_nav_cost_fields(ref(G(**grid)), ref(S(**{**seed, **bad})), None) == -1, bad
    both = (dict(n_points=0), dict(n_points=-1), dict(n_goals=0), dict(n_goals=-3), dict(points=None), dict(fields=None), dict(n_points=2),
            dict(points=68), dict(fields=66), dict(goal=66))
    for bad in both + (dict(lookahead=0), dict(lookahead=-1), dict(lookahead=65), dict(waypoints=None), dict(waypoints=68), dict(hops=66)):
        assert h.ms_nav_cost_waypoints(ref(G(**grid)), ref(W(**{**way, **bad})), None) == -1, bad
    for bad in both + (dict(max_points=1), dict(max_points=0), dict(max_points=-4), dict(paths=None), dict(counts=None), dict(paths=66),
                       dict(counts=66)):
        assert h.ms_nav_cost_paths(ref(G(**grid)), ref(P(**{**path, **bad})), None) == -1, bad
    # the host instantiations
    c = costed()[0]
    case = c.case
    geom, free, marks = np.array(case.geom, np.int32), np.ascontiguousarray(case.free, np.uint8), np.ascontiguousarray(case.marks, np.uint8)
    D = np.zeros(case.free.shape, F)
    ptr = lambda a: a.ctypes.data
    args = lambda **kw: [kw.get('geom', ptr(geom)), kw.get('cell', CELL), kw.get('free', ptr(free)), kw.get('marks', ptr(marks)),
                         kw.get('where', 1), None, kw.get('cost', ptr(c.cost)), 0, kw.get('D', ptr(D)), None]
    assert h.ms_host_nav_cost_field(*args()) > 0
    for bad in (dict(geom=None), dict(cell=0.), dict(cell=float('inf')), dict(where=2), dict(where=-1), dict(free=None), dict(marks=None), dict(D=None),
                dict(cost=None)):
        assert h.ms_host_nav_cost_field(*args(**bad)) == -1, bad
    p = case.points[0]
    assert host_cost_follow(c.world, c.cost, p, lookahead=0)[1] == -2 and host_cost_follow(c.world, c.cost, p, lookahead=65)[1] == -2
    assert host_cost_follow(c.world, c.cost, p, max_points=1)[1] == 0
    g, f, d, q = (np.ascontiguousarray(a) for a in (geom, free, c.D, np.asarray(p, F)))
    out = np.zeros(8, F)
    assert h.ms_host_nav_cost_waypoint(ptr(g), CELL, ptr(f), ptr(d), None, ptr(q), 16, ptr(out)) == -1 and np.isnan(out[:2]).all()
    assert h.ms_host_nav_cost_path(ptr(g), CELL, ptr(f), ptr(d), None, ptr(q), 4, ptr(out)) == 0 and np.isnan(out).all()


def _cpu_grid():
    from megastep_amd import cuda
    geom = np.array([[0, 0, 8, 8], [0, 0, 8, 8]], np.int32)
    starts = np.array([0, 64, 128], np.int64)
    return cuda.NavGrid(torch.as_tensor(geom), torch.as_tensor(starts), torch.ones(128, dtype=torch.uint8), CELL, RADIUS, geom, starts)


def test_the_python_calls_refuse_what_they_cannot_do():
    from megastep_amd import cuda
    grid = _cpu_grid()
    marks = torch.zeros(3*128, dtype=torch.uint8)
    shared, own = torch.ones(128), torch.ones(3*128)
    for cost in (shared, own, cuda.cell_layer(own, 3), cuda.cell_layer(shared)):
        with pytest.raises(RuntimeError, match='GPU'):
            cuda.cost_fields(grid, marks, 3, cost)
    with pytest.raises(RuntimeError, match='GPU'):
        cuda.cost_fields(grid, marks.bool(), 3, shared, where=False, among=torch.ones(128, dtype=torch.bool))
    with pytest.raises(RuntimeError, match='GPU'):
        cuda.seen_maps(grid, 3).frontier_fields(cost=shared)
    for bad in (0, -1, 2.5):
        with pytest.raises(RuntimeError, match='n_fields'):
            cuda.cost_fields(grid, marks, bad, shared)
    with pytest.raises(RuntimeError, match='entries'):
        cuda.cost_fields(grid, marks, 2, shared)
    for bad in (marks.float(), marks.reshape(3, 128), list(range(4))):
        with pytest.raises(RuntimeError, match='marks'):
            cuda.cost_fields(grid, bad, 3, shared)
    for bad in (torch.ones(64, dtype=torch.uint8), torch.ones(128)):
        with pytest.raises(RuntimeError, match='among'):
            cuda.cost_fields(grid, marks, 3, shared, among=bad)
    for bad in (torch.ones(2*128), torch.ones(127), shared.double(), shared.to(torch.uint8), own.reshape(3, 128), own[::3], [1.]*128,
                cuda.cell_layer(torch.ones(2*128), 2), cuda.cell_layer(torch.ones(128, dtype=torch.uint8)),
                cuda.cell_layer(own, 3, field=torch.zeros(2, 3, dtype=torch.int32))):
        with pytest.raises(RuntimeError, match='cost|layer'):
            cuda.cost_fields(grid, marks, 3, bad)
    fields = cuda.CostFields(grid, marks, 3, True, None, own, 3, torch.zeros(3*128), torch.zeros(2, 3, dtype=torch.int32))
    assert isinstance(fields, cuda.SeededFields) and fields.n_goals == fields.n_fields == 3 and fields.image(1, 2).shape == (8, 8)
    assert fields.cost is own and fields.n_costs == 3
    with pytest.raises(RuntimeError, match='unweighted hop'):
        fields.basins()
    with pytest.raises(RuntimeError, match='unweighted hop'):
        fields.basins(ids=None, n_ids=0)
    for call in (lambda: cuda.basins(fields), lambda: cuda.basins(fields, n_ids=2, passes=True), lambda: cuda.SeededFields.basins(fields)):
        with pytest.raises(RuntimeError, match='unweighted hop'):                 # (the function itself, not only the method)
            call()
    for bad in (torch.ones(2, 3), torch.ones(3, 2, dtype=torch.bool)):
        with pytest.raises(RuntimeError, match='mask'):
            fields.update(bad)
    with pytest.raises(RuntimeError, match='GPU'):
        fields.update()
    with pytest.raises(RuntimeError, match='`out`'):
        cuda.cost_fields(grid, marks, 3, own.clone(), out=fields)
    with pytest.raises(RuntimeError, match='`out`'):
        cuda.cost_fields(grid, marks, 3, own, where=False, out=fields)
    with pytest.raises(RuntimeError, match='`out`'):
        cuda.cost_fields(grid, marks, 3, own, out=cuda.SeededFields(grid, marks, 3, True, None, fields.values, fields.n_seeds))
    pts = torch.zeros(2, 3, 2)
    for call in (fields.at, fields.waypoints, fields.paths):
        with pytest.raises(RuntimeError, match='GPU'):
            call(pts)
        with pytest.raises(RuntimeError, match=r'\(N, P, 2\)'):
            call(torch.zeros(3, 3, 2))
        with pytest.raises(RuntimeError, match='one per field'):
            call(torch.zeros(2, 5, 2))
    for bad in (0, 65, 2.5):
        with pytest.raises(RuntimeError, match='lookahead'):
            fields.waypoints(pts, lookahead=bad)
    # SeededFields keeps its positional signature
    plain = cuda.SeededFields(grid, marks, 3, True, None, torch.zeros(3*128), torch.zeros(2, 3, dtype=torch.int32))
    assert plain.passes is None and not isinstance(plain, cuda.CostFields)


def test_the_builders_formulas_hold_on_hand_values():
    from megastep_amd import cuda
    d = torch.tensor([0., .125, .25, .375, .5, .75, 2., float('inf'), float('nan')])
    got = cuda.inflation_costs(d, .5)
    assert got[:8].tolist() == [5., 4., 3., 2., 1., 1., 1., 1.] and torch.isnan(got[8])
    assert np.array_equal(bits(got.numpy()), bits(inflation(d.numpy(), .5)))
    assert cuda.inflation_costs(d, .25, weight=8.)[:3].tolist() == [9., 5., 1.]
    assert cuda.inflation_costs(d, .5, weight=0.)[:8].tolist() == [1.]*8
    rng = np.random.RandomState(1)
    many = rng.uniform(0, 1, 500).astype(F)
    assert np.array_equal(bits(cuda.inflation_costs(torch.as_tensor(many), .3, 4.).numpy()), bits(inflation(many, .3)))
    out = torch.zeros(9)
    assert cuda.inflation_costs(d, .5, out=out) is out and out[:3].tolist() == [5., 4., 3.]
    with pytest.raises(RuntimeError, match='`out`'):
        cuda.inflation_costs(d, .5, out=d)
    for bad in (dict(radius=0.), dict(radius=float('inf')), dict(radius=-1.), dict(radius=.5, weight=-1.), dict(radius=.5, weight=float('nan'))):
        with pytest.raises(RuntimeError, match='radius'):
            cuda.inflation_costs(d, **bad)
    with pytest.raises(RuntimeError, match='clear'):
        cuda.inflation_costs(d.double(), .5)
    with pytest.raises(RuntimeError, match='`out`'):
        cuda.inflation_costs(d, .5, out=torch.zeros(8))
    # a NaN clearance is the dearest cell: the clamp of the multiplier, not of the builder
    assert cost_rule.multiplier(got.numpy())[8] == 256
    m = torch.tensor([0, 1, 2, 255, 0], dtype=torch.uint8)
    assert cuda.mark_costs(m).tolist() == [256., 1., 1., 1., 256.] and cuda.mark_costs(m).dtype == torch.float32
    assert cuda.mark_costs(m, where=False).tolist() == [1., 256., 256., 256., 1.]
    assert cuda.mark_costs(m.bool(), on=8., off=2.).tolist() == [2., 8., 8., 8., 2.]
    assert np.array_equal(cuda.mark_costs(m, on=8., off=2.).numpy(), marked(m.numpy(), 8., 2.))
    gate = torch.tensor([1, 0, 1, 0, 0], dtype=torch.uint8)
    assert cuda.mark_costs(m, on=8., off=2., gate=gate).tolist() == [2., 1., 8., 1., 1.]
    out = torch.zeros(5)
    assert cuda.mark_costs(m, out=out) is out and out.tolist() == [256., 1., 1., 1., 256.]
    grid = _cpu_grid()
    maps = cuda.seen_maps(grid, 3)
    maps.values[5] = 1
    known = cuda.mark_costs(maps)
    assert known.shape == (3*128,) and known[5] == 1 and (known == 256).sum() == 3*128 - 1
    for bad in (dict(layer=torch.ones(5)), dict(layer=m, gate=torch.ones(5)), dict(layer=m, gate=gate[:4])):
        with pytest.raises(RuntimeError, match='byte layer'):
            cuda.mark_costs(**bad)


def test_routes_and_the_new_keywords_default_to_todays_behaviour():
    import inspect
    from megastep_amd import cuda, modules
    from megastep_amd.demo.envs.pointgoal import PointGoal
    assert list(inspect.signature(modules.Routes.__init__).parameters) == ['self', 'core', 'grid', 'goals', 'cost']
    assert inspect.signature(modules.Frontiers.__init__).parameters['cost'].default is None
    assert inspect.signature(PointGoal.__init__).parameters['margin'].default is None
    assert inspect.signature(cuda.SeenMaps.frontier_fields).parameters['cost'].default is None
    routes = modules.Routes(None, None, None, None)
    assert routes.seeds is None and routes.fields is None
    assert all(hasattr(modules.Routes, name) for name in ('waypoints', 'distances', '__call__'))
