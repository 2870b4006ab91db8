"""Pulled paths (`ms_nav_pulls`, `DistanceFields.pulled` / `SeededFields.pulled` / `CostFields.pulled`, `modules.SPL`,
`PointGoal(spl=True)`) on the CPU: the contract of include/megastep_hip.h (MsNavPulls) restated in binary32 numpy (`pull_rule`,
built on path_rule's chain and sight, which tests/test_gpu_navpull.py holds the kernel to, bit for bit); the serial host statement
of the rule over the kernels' own device functions (`ms_host_nav_pull`) against it; what the rule promises - no segment through a
wall, a length between the straight line and the chain's, most paths shortened by 2 % or more; hand-made grids at the sizes where
a wave's bookkeeping can go wrong; the C-ABI's declarations, layout and refusals; and SPL's arithmetic."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests.test_abi import ROOT, declared_symbols
from tests.test_navfield_host import CELL, CELLS, F, INF, RADIUS, _crossings, bits, nav_rule
from tests.test_navpath_host import NAN, cases, path_rule

REACHES = (1, 2, 16, 63, 64, 65, 256, 1024)
MAX_POINTS = (2, 8, 64)


class pull_rule:
    """The contract in numpy: path_rule's chain (seed_rule's on a seeded or a cost field) and path_rule's sight, every operation
    one binary32 operation, in the order the header gives."""

    @staticmethod
    def pull(world, p, reach, table=None, chain=path_rule.chain):
        """(P [(x, y)], V [index], ended): the points P_0 = p, P_1 = x_0, ... of the whole path and the indices the pull keeps;
        None without a path."""
        found = chain(world, p, None, table)
        if found is None:
            return None
        points, ended, _, _ = found
        P = [(F(p[0]), F(p[1]))] + points
        sighted = (world[0], world[1], world[2], world[3], None)         # (what path_rule.sights reads: the grid and its free cells)
        n, a, V = len(P), 0, [0]
        while a < n - 1:
            hi, k = min(a + reach, n - 1), a + 1
            if hi > a + 1:
                xs, ys = (np.array([pt[c] for pt in P[a + 2:hi + 1]], F) for c in (0, 1))
                admissible = np.nonzero(path_rule.sights(sighted, P[a], xs, ys))[0]
                if len(admissible):
                    k = a + 2 + int(admissible[-1])
            V.append(k)
            a = k
        return P, V, ended

    @staticmethod
    def length(vertices):
        """From +0.f, in vertex order: L = fl(L + sqrtf(fl(fl(dx*dx) + fl(dy*dy))))."""
        L = F(0)
        for (ax, ay), (bx, by) in zip(vertices[:-1], vertices[1:]):
            dx, dy = F(bx) - F(ax), F(by) - F(ay)
            L = F(L + np.sqrt(F(F(dx*dx) + F(dy*dy))))
        return L

    @staticmethod
    def outputs(found, max_points):
        """MsNavPulls' outputs of one query: (vertices (M, 2), indices (M,), counts, cells, lengths)."""
        vertices, indices = np.full((max_points, 2), NAN, F), np.full(max_points, -1, np.int32)
        if found is None:
            return vertices, indices, 0, 0, INF
        P, V, ended = found
        m = min(len(V), max_points)
        vertices[:m] = np.array([P[k] for k in V[:m]], F)
        indices[:m] = V[:m]
        sign = 1 if ended else -1
        return vertices, indices, sign*len(V), sign*len(P), pull_rule.length([P[k] for k in V])


_SPARE = np.zeros(8, np.uint8)


def host_pull(world, p, reach, max_points, cost=None, indices=True):
    """ms_host_nav_pull on a path_rule world (a goal) or a seed_rule world (none): (vertices, indices or None, counts, length)."""
    from megastep_amd import _lib
    h = _lib.lib()
    geom, cell, free, D = world[:4]
    q = None if len(world) < 5 or world[4] is None else np.ascontiguousarray(world[4], F)
    geom = np.array(geom, np.int32)
    free, D, p = np.ascontiguousarray(free, np.uint8), np.ascontiguousarray(D, F), np.ascontiguousarray(p, F)
    cost = None if cost is None else np.ascontiguousarray(cost, F)
    ptr = lambda a: None if a is None else (a.ctypes.data or _SPARE.ctypes.data)
    vertices = np.zeros((max(max_points, 0), 2), F)
    chosen = np.full(max(max_points, 0), -7, np.int32) if indices else None
    length = ctypes.c_float(-7.)
    count = h.ms_host_nav_pull(ptr(geom), cell, ptr(free), ptr(D), ptr(q), ptr(cost), ptr(p), reach, max_points, ptr(vertices), ptr(chosen),
                               ctypes.addressof(length))
    return vertices, chosen, count, F(length.value)


def _same(world, p, table, reaches=(64,), max_points=(8,), chain=path_rule.chain, cost=None):
    """The host statement against the rule for every reach and max_points; returns the rule's (counts, cells) at the last reach."""
    for R in reaches:
        found = pull_rule.pull(world, p, R, table, chain)
        for M in max_points:
            want_v, want_i, want_count, want_cells, want_L = pull_rule.outputs(found, M)
            got_v, got_i, got_count, got_L = host_pull(world, p, R, M, cost)
            assert got_count == want_count, (p, R, M, got_count, want_count)
            assert np.array_equal(bits(got_v), bits(want_v)) and np.array_equal(got_i, want_i), (p, R, M)
            assert bits(got_L) == bits(want_L), (p, R, M, got_L, want_L)
    return want_count, want_cells


def _odd_points(walls):
    """Points in walls, outside the grid, not numbers."""
    lo, hi = walls.reshape(-1, 2).min(0), walls.reshape(-1, 2).max(0)
    rng = np.random.RandomState(5)
    odd = [walls.reshape(-1, 2, 2).mean(1)[k] for k in range(0, len(walls), 7)]
    odd += list(lo - .3 + rng.uniform(0, 1, (40, 2))*(hi - lo + .6))
    return odd + [lo - 5., hi + 1e6, [np.nan, 2.], [2., np.inf], [-3e38, 3e38]]


# ---------------------------------------------------------------------------------------------------------------------
# 1. the host statement is the rule, bit for bit: fields of goals, seeded fields, cost fields
# ---------------------------------------------------------------------------------------------------------------------
def _host_pull_is_the_rule(found):
    cut = long = 0
    for case in found:
        for k, p in enumerate(case.points):
            count, cells = _same(case.world, p, case.table, REACHES if k % 4 == 0 else (64,), MAX_POINTS)
            cut += count > 8
            long += cells > 65
        none = 0
        for p in _odd_points(case.walls):
            p = np.array(p, F)
            count, cells = _same(case.world, p, case.table, (1, 64, 1024), (2, 8))
            if count == 0:
                none += 1
                vertices, chosen, _, length = host_pull(case.world, p, 64, 4)
                assert cells == 0 and np.isnan(vertices).all() and (chosen == -1).all() and length == INF and length > 0
        assert 5 <= none
    # the inputs exercise what they are there for (by the rule alone): paths cut at 8 vertices, chains longer than a window of 64 -
    # fewer of those at the widest cell, whose chains have 5/8 of the points
    assert cut > 50 and long > 50, (cut, long)


def test_the_host_pull_is_the_rule_bit_for_bit():
    _host_pull_is_the_rule(cases())


@pytest.mark.parametrize('cell,r', CELLS)
def test_the_host_pull_is_the_rule_at_other_cell_widths(cell, r):
    _host_pull_is_the_rule(cases(cell, r))


def test_the_host_pull_is_the_rule_on_seeded_fields():
    from tests.test_navseed_host import cases as seeded, seed_rule
    compared = 0
    for case in seeded():
        if not case.seeds.any():
            continue
        for k, p in enumerate(case.points[::9]):
            p = (p + F(.03)).astype(F)
            count, cells = _same(case.world, p, case.table, REACHES if k % 4 == 0 else (64,), MAX_POINTS, chain=seed_rule.chain)
            compared += count > 0
        for p in _odd_points(case.walls)[::5]:
            _same(case.world, np.array(p, F), case.table, (1, 64), (2, 8), chain=seed_rule.chain)
    assert compared > 100, compared


def test_the_host_pull_is_the_rule_on_cost_fields():
    from tests.test_navcost_host import costed, cost_rule
    from tests.test_navseed_host import seed_rule
    compared = bent = 0
    for c in costed():
        if not c.case.seeds.any():
            continue
        unweighted = seed_rule.hops(c.world)
        for k, p in enumerate(c.case.points[::17]):
            p = (p + F(.03)).astype(F)
            count, cells = _same(c.world, p, c.table, REACHES if k % 4 == 0 else (64,), (2, 64), chain=cost_rule.chain, cost=c.cost)
            compared += count > 0
            # (the comparison would pass on a kernel that ignores the costs unless the unweighted hop goes another way somewhere)
            other = pull_rule.outputs(pull_rule.pull(c.world, p, 64, unweighted, seed_rule.chain), 64)
            mine = pull_rule.outputs(pull_rule.pull(c.world, p, 64, c.table, cost_rule.chain), 64)
            bent += other[2] != mine[2] or not np.array_equal(bits(other[0]), bits(mine[0]))
    assert compared > 100 and bent > 0, (compared, bent)


# ---------------------------------------------------------------------------------------------------------------------
# 2. reach = 1 is the chain itself
# ---------------------------------------------------------------------------------------------------------------------
def test_a_reach_of_one_gives_the_chain_and_its_length_is_the_query():
    paths = 0
    for case in cases():
        for p, g in zip(case.points, case.g):
            want, count = path_rule.path(case.world, p, 256, case.table)
            got, chosen, got_count, L = host_pull(case.world, p, 1, 256)
            assert got_count == count and np.array_equal(bits(got), bits(want))
            # (at reach 1 every point is a vertex: counts is MsNavPaths' count, which is what `cells` reports at any reach)
            assert pull_rule.outputs(pull_rule.pull(case.world, p, 64, case.table), 2)[3] == count
            assert np.array_equal(chosen[:min(count, 256)], np.arange(min(count, 256)))
            if count == 0:
                assert L == INF and not np.isfinite(g)
                continue
            paths += 1
            assert count > 0 and abs(float(L) - float(g)) <= count*2.**-23*max(float(L), 1.), (L, g, count)
    assert paths > 300


# ---------------------------------------------------------------------------------------------------------------------
# 3. what the rule promises, by the numpy rule alone
# ---------------------------------------------------------------------------------------------------------------------
def _geometry(found, reach=64):
    """(ratios pulled/chain, most vertices, segments, crossings) over the cases' starts that have a path."""
    ratios, most, segments, crossings = [], 0, 0, 0
    for case in found:
        starts, ends = [], []
        for p in case.points:
            pulled = pull_rule.pull(case.world, p, reach, case.table)
            if pulled is None:
                continue
            P, V, ended = pulled
            assert ended and V[0] == 0 and V[-1] == len(P) - 1 and all(0 < b - a <= reach for a, b in zip(V[:-1], V[1:]))
            vertices = np.array([P[k] for k in V], np.float64)
            L = float(pull_rule.length([P[k] for k in V]))
            chain = float(pull_rule.length(P))
            straight = float(np.linalg.norm(vertices[-1] - vertices[0]))
            assert L <= chain*(1 + 1e-6) and L >= straight*(1 - 1e-6), (L, chain, straight)
            ratios.append(L/chain)
            most = max(most, len(V))
            starts += list(vertices[:-1]); ends += list(vertices[1:])
        segments += len(starts)
        crossings += _crossings(np.array(starts), np.array(ends), case.walls)
    return np.array(ratios), most, segments, crossings


def test_pulled_paths_cross_no_wall_and_most_are_two_per_cent_shorter_than_the_chain():
    ratios, most, segments, crossings = _geometry(cases())
    print(f'{len(ratios)} paths, {segments} segments, {crossings} crossings; pulled/chain: mean {ratios.mean():.4f}, min {ratios.min():.4f}, '
          f'max {ratios.max():.6f}; shortened by 2 % or more: {(ratios <= .98).mean():.3f}; vertices at most {most}')
    assert len(ratios) > 300 and segments > 2000
    assert crossings == 0
    assert ratios.mean() <= .96
    assert (ratios <= .98).mean() >= .9


@pytest.mark.parametrize('cell,r', CELLS)
def test_pulled_paths_at_other_cell_widths(cell, r):
    ratios, most, segments, crossings = _geometry(cases(cell, r))
    print(f'cell {cell}: {len(ratios)} paths, {segments} segments, {crossings} crossings; pulled/chain: mean {ratios.mean():.4f}; shortened '
          f'by 2 % or more: {(ratios <= .98).mean():.3f}; vertices at most {most}')
    assert len(ratios) > 250 and crossings == 0
    assert ratios.mean() <= .96
    assert (ratios <= .98).mean() >= .9


# ---------------------------------------------------------------------------------------------------------------------
# 4. hand-made grids: the smallest shapes where the bookkeeping of a window, a ring and a batch of candidates can go wrong
# ---------------------------------------------------------------------------------------------------------------------
def centre(i, j, cell=CELL):
    return np.array([(F(j) + F(.5))*F(cell), (F(i) + F(.5))*F(cell)], F)


def grid_world(free, q, cell=CELL):
    """A path_rule world on a hand-made grid whose cell (0, 0) has its corner at the origin."""
    geom = (0, 0, free.shape[1], free.shape[0])
    q = np.array(q, F)
    return geom, cell, free, nav_rule.field(free, geom, cell, q), q


def room():
    """An empty room of 40 x 40 free cells, a start and a goal well inside it."""
    free = np.zeros((42, 42), bool); free[1:41, 1:41] = True
    return grid_world(free, (4.1, 3.3)), np.array([.7, .9], F)


def corner():
    """An L-shaped corridor three cells wide: along the bottom, then up the right-hand side."""
    free = np.zeros((24, 24), bool)
    free[1:4, 1:23] = True
    free[1:23, 20:23] = True
    return grid_world(free, centre(20, 21) + F(.01)), (centre(2, 2) + F(.02)).astype(F)


def corridor(n):
    """A straight corridor three cells wide whose chain from the start has exactly n points (p, n - 2 cells, q), n >= 3."""
    free = np.zeros((5, n + 3), bool); free[1:4, 1:n + 2] = True
    return grid_world(free, centre(2, n - 1)), centre(2, 2)


CORRIDORS = (3, 4, 64, 65, 66, 67, 256, 300)                            # reach + 1, reach + 2 and >= 4 reach for reach 1 and 64


def seeded_on_a_seed():
    """A seeded field whose start stands by a seed: the chain is [x_0]."""
    free = np.zeros((8, 8), bool); free[1:7, 1:7] = True
    D = np.full((8, 8), INF, F)
    D[3, 3] = 0
    D[3, 4] = D[4, 3] = D[2, 3] = D[3, 2] = F(CELL)
    return ((0, 0, 8, 8), CELL, free, D), (centre(3, 3) + F(.01)).astype(F)


def constant():
    """A field overwritten with a constant: no neighbour is below any cell."""
    world, p = room()
    return (world[0], world[1], world[2], np.where(world[2], F(3), INF).astype(F), world[4]), p


def test_an_empty_room_is_one_segment():
    world, p = room()
    found = pull_rule.pull(world, p, 64)
    assert found[1] == [0, len(found[0]) - 1] and 20 < len(found[0]) <= 65
    vertices, chosen, count, L = host_pull(world, p, 64, 8)
    assert count == 2 and chosen.tolist() == [0, len(found[0]) - 1] + [-1]*6
    assert np.array_equal(bits(vertices[:2]), bits(np.array([p, world[4]]))) and np.isnan(vertices[2:]).all()
    dx, dy = world[4][0] - p[0], world[4][1] - p[1]
    assert bits(L) == bits(np.sqrt(F(F(dx*dx) + F(dy*dy))))
    _same(world, p, None, REACHES, MAX_POINTS)


def test_an_l_shaped_corridor_has_one_corner_and_it_is_a_cell_of_the_chain():
    world, p = corner()
    P, V, ended = pull_rule.pull(world, p, 64)
    assert ended and len(V) == 3 and 1 < V[1] < len(P) - 1 and len(P) <= 65
    vertices, chosen, count, L = host_pull(world, p, 64, 8)
    assert count == 3 and chosen[:3].tolist() == V
    i, j = path_rule.chain(world, p)[3][V[1] - 1]
    assert np.array_equal(bits(vertices[1]), bits(centre(i, j)))
    assert L < pull_rule.length(P)                                       # (two straight segments against the chain's staircase)
    _same(world, p, None, REACHES, MAX_POINTS)


def test_a_start_on_a_seed_has_two_points():
    from tests.test_navseed_host import seed_rule
    world, p = seeded_on_a_seed()
    P, V, ended = pull_rule.pull(world, p, 64, chain=seed_rule.chain)
    assert ended and len(P) == 2 and V == [0, 1]
    vertices, chosen, count, L = host_pull(world, p, 64, 4)
    assert count == 2 and np.array_equal(bits(vertices[:2]), bits(np.array([p, centre(3, 3)])))
    _same(world, p, None, (1, 64, 1024), MAX_POINTS, chain=seed_rule.chain)


@pytest.mark.parametrize('n', CORRIDORS)
def test_straight_corridors_at_the_windows_edges(n):
    world, p = corridor(n)
    for reach in (1, 64):
        P, V, ended = pull_rule.pull(world, p, reach)
        assert ended and len(P) == n
        # down the middle of three free rows everything is in sight: every vertex is the window's far end, but the last
        assert V == list(range(0, n - 1, reach)) + [n - 1]
        count, cells = _same(world, p, None, (reach,), (2, 8, 512))
        assert (count, cells) == (len(V), n)
    _same(world, p, None, (2, 63, 65, 256, 1024), (8,))


def test_a_constant_field_breaks_the_chain_and_the_call_returns():
    world, p = constant()
    assert _same(world, p, None, (1, 64, 1024), MAX_POINTS) == (-2, -2)
    vertices, chosen, count, L = host_pull(world, p, 64, 4)
    assert count == -2 and np.isfinite(L) and np.array_equal(bits(vertices[0]), bits(p)) and np.isnan(vertices[2:]).all()
    # garbage: NaNs, infinities and negative numbers over a field
    case = cases()[3]
    rng = np.random.RandomState(3)
    D = case.D.copy()
    D[rng.rand(*D.shape) < .05] = np.nan
    D[rng.rand(*D.shape) < .05] = -np.inf
    D[rng.rand(*D.shape) < .05] = -2.
    junk = (case.geom, CELL, case.free, D, case.goal)
    table = path_rule.hops(junk)
    broken = sum(_same(junk, p, table, (1, 64, 256), (8, 64))[0] < 0 for p in case.points[:30])
    assert broken > 5


# ---------------------------------------------------------------------------------------------------------------------
# 5. header, loader, refusals
# ---------------------------------------------------------------------------------------------------------------------
FIELDS = ('n_points', 'points', 'goal', 'fields', 'goals', 'n_goals', 'costs', 'n_costs', 'reach', 'max_points', 'mask', 'vertices', 'indices',
          'counts', 'cells', 'lengths')


def test_the_header_declares_the_pull_calls_and_the_loader_binds_them():
    from megastep_amd import _lib
    assert 'ms_nav_pulls' in declared_symbols(('megastep_hip.h',))
    assert {'ms_host_nav_pull', 'ms_debug_nav_pull_scheme'} <= set(declared_symbols(('megastep_hip_test.h',)))
    assert {'ms_nav_pulls', 'ms_host_nav_pull', 'ms_debug_nav_pull_scheme'} <= set(_lib.SYMBOLS)
    text = open(os.path.join(ROOT, 'include', 'megastep_hip.h')).read()
    assert int(re.search(r'#define MS_ABI_VERSION (\d+)', text).group(1)) == _lib.ABI_VERSION == 17
    handle = _lib.lib()
    assert hasattr(handle, 'ms_nav_pulls') and hasattr(handle, 'ms_host_nav_pull') and handle.ms_abi_version() == 17
    assert handle.ms_debug_nav_pull_scheme(2) == -1 and handle.ms_debug_nav_pull_scheme(-2) == -1
    assert handle.ms_debug_nav_pull_scheme(1) == 0 and handle.ms_debug_nav_pull_scheme(-1) == 0


def test_the_pull_mirror_has_the_c_layout():
    import subprocess
    import tempfile
    from megastep_amd import _lib
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "megastep_hip.h"\nint main(){printf("%zu", sizeof(MsNavPulls));' +
           ''.join(f'printf(" %zu", offsetof(MsNavPulls, {f}));' for f in FIELDS) + '}')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, 't.c'), 'w').write(src)
        subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), os.path.join(d, 't.c'), '-o', os.path.join(d, 't')])
        got = list(map(int, subprocess.check_output([os.path.join(d, 't')]).split()))
    mirror = _lib.MsNavPulls
    assert [f for f, _ in mirror._fields_] == list(FIELDS)
    assert got == [ctypes.sizeof(mirror)] + [getattr(mirror, f).offset for f in FIELDS]


def test_bad_pull_arguments_are_refused_before_any_launch():
    from megastep_amd import _lib
    h = _lib.lib()
    fake = 64                                       # (never dereferenced: every call below fails its checks first)
    grid = dict(n_envs=2, cell=.125, clearance=.106, geom=fake, starts=fake, max_framed=100, free_cells=fake)
    pull = dict(n_points=1, points=fake, goal=None, fields=fake, goals=fake, n_goals=1, costs=None, n_costs=0, reach=64, max_points=8,
                mask=None, vertices=fake, indices=None, counts=fake, cells=None, lengths=fake)
    G, P = _lib.MsNavGrid, _lib.MsNavPulls
    ref = ctypes.byref
    assert h.ms_nav_pulls(None, ref(P(**pull)), None) == -1
    assert h.ms_nav_pulls(ref(G(**grid)), None, None) == -1
    for bad in (dict(n_envs=0), dict(cell=0.), dict(cell=float('nan')), dict(clearance=0.), dict(cell=.15), dict(geom=None),
                dict(starts=None), dict(free_cells=None), dict(max_framed=-1), dict(geom=68)):
        assert h.ms_nav_pulls(ref(G(**{**grid, **bad})), ref(P(**pull)), None) == -1, bad
    for bad in (dict(n_points=0), dict(n_points=-1), dict(n_goals=0), dict(n_goals=-3), dict(points=None), dict(fields=None), dict(n_points=2),
                dict(points=68), dict(goals=68), dict(fields=66), dict(goal=66),
                dict(reach=0), dict(reach=-1), dict(reach=1025), dict(max_points=1), dict(max_points=0), dict(max_points=-4),
                dict(max_points=2**20 + 1),
                dict(n_costs=1), dict(n_costs=-1), dict(costs=fake), dict(costs=fake, n_costs=2), dict(costs=fake, n_costs=-1),
                dict(costs=66, n_costs=1), dict(costs=fake, n_costs=3, n_goals=2, goal=fake),
                dict(vertices=None), dict(counts=None), dict(lengths=None), dict(vertices=66), dict(indices=66), dict(counts=66),
                dict(cells=66), dict(lengths=66)):
        assert h.ms_nav_pulls(ref(G(**grid)), ref(P(**{**pull, **bad})), None) == -1, bad
    # the host statement: a reach out of range; fewer than two vertices, or nowhere to write
    world, p = room()
    for reach in (0, -1, 1025):
        assert host_pull(world, p, reach, 8)[2] == -2
    vertices, chosen, count, L = host_pull(world, p, 64, 1)
    assert count == 0 and L == F(-7.)
    assert host_pull(world, p, 64, 8, indices=False)[2] == 2            # (indices are optional)


def test_the_python_calls_refuse_what_they_cannot_do():
    from megastep_amd import cuda
    geom = np.array([[0, 0, 8, 8], [0, 0, 8, 8]], np.int32)
    starts = np.array([0, 64, 128], np.int64)
    grid = cuda.NavGrid(torch.as_tensor(geom), torch.as_tensor(starts), torch.ones(128, dtype=torch.uint8), CELL, RADIUS, geom, starts)
    fields = cuda.DistanceFields(grid, torch.zeros(2, 3, 2), torch.zeros(3*128))
    seeded = cuda.SeededFields(grid, torch.zeros(3*128, dtype=torch.uint8), 3, True, None, torch.zeros(3*128), torch.zeros(2, 3, dtype=torch.int32))
    costs = cuda.CostFields(grid, torch.zeros(3*128, dtype=torch.uint8), 3, True, None, torch.ones(128), 1, torch.zeros(3*128),
                            torch.zeros(2, 3, dtype=torch.int32))
    pts = torch.zeros(2, 3, 2)
    for owner in (fields, seeded, costs):
        call = owner.pulled
        with pytest.raises(RuntimeError, match='GPU'):
            call(pts)
        with pytest.raises(RuntimeError, match=r'\(N, P, 2\)'):
            call(torch.zeros(3, 3, 2))
        with pytest.raises(RuntimeError, match='dtype'):
            call(pts.double())
        with pytest.raises(RuntimeError, match='one per field'):
            call(torch.zeros(2, 5, 2))
        with pytest.raises(RuntimeError, match='integer'):
            call(pts, goal=torch.zeros(2, 3))
        for bad in (0, 1025, 2.5, -1):
            with pytest.raises(RuntimeError, match='reach'):
                call(pts, reach=bad)
        for bad in (1, 0, 3., 2**20 + 1):
            with pytest.raises(RuntimeError, match='max_points'):
                call(pts, max_points=bad)
        for bad in (torch.zeros(2, 4, dtype=torch.bool), torch.zeros(2, 3), torch.zeros(3, 3, dtype=torch.bool)):
            with pytest.raises(RuntimeError, match='mask'):
                call(pts, mask=bad)
        held = cuda.PulledPaths(torch.zeros(2, 3, 8, 2), torch.zeros(2, 3, dtype=torch.int32), torch.zeros(2, 3), torch.zeros(2, 3, dtype=torch.int32))
        for kw in (dict(max_points=16), dict(max_points=8, indices=True)):
            with pytest.raises(RuntimeError, match='out'):
                call(pts, out=held, **kw)
        with pytest.raises(RuntimeError, match='out'):
            call(pts, max_points=8, out=cuda.Paths(held.points, held.counts))
        with pytest.raises(RuntimeError, match='GPU'):
            call(pts, max_points=8, out=held)                           # (the right shape: what is wrong is where it lives)
    assert issubclass(cuda.PulledPaths, cuda.Paths) and held.path(0, 0).shape == (0, 2)


# ---------------------------------------------------------------------------------------------------------------------
# 6. SPL's arithmetic
# ---------------------------------------------------------------------------------------------------------------------
def test_spl_scores_an_episode_by_its_shortest_path_over_what_was_walked():
    from megastep_amd import modules
    inf, nan = float('inf'), float('nan')
    #                         walked more   walked less   on the dot   not arrived  not ended  no path  no path, not ended  NaN walked
    shortest = torch.tensor([[4., 4., 4., 4., 4., inf, inf, 4.]])
    walked = torch.tensor([[5., 3., 4., 5., 5., 5., 5., nan]])
    arrived = torch.tensor([[True, True, True, False, True, True, False, False]])
    ended = torch.tensor([[True, True, True, True, False, True, False, True]])
    got = modules.SPL.score(shortest, walked, arrived, ended)
    assert got.dtype == torch.float32 and got.shape == (1, 8)
    assert torch.equal(got[0, :4], torch.tensor([.8, 1., 1., 0.])) and got[0, 7].item() == 0.
    assert torch.isnan(got[0, 4:7]).all()
    # NaN exactly where no episode ended or the shortest path is not finite; within [0, 1] elsewhere
    rng = np.random.RandomState(2)
    shortest = torch.as_tensor(np.where(rng.rand(64, 3) < .1, np.inf, rng.uniform(.5, 20, (64, 3))).astype(F))
    walked = torch.as_tensor(rng.uniform(0, 30, (64, 3)).astype(F))
    arrived, ended = torch.as_tensor(rng.rand(64, 3) < .5), torch.as_tensor(rng.rand(64, 3) < .5)
    got = modules.SPL.score(shortest, walked, arrived, ended)
    assert torch.equal(torch.isnan(got), ~ended | ~torch.isfinite(shortest))
    scored = got[~torch.isnan(got)]
    assert ((scored >= 0) & (scored <= 1)).all() and (scored == 1).any() and (scored == 0).any() and ((scored > 0) & (scored < 1)).any()
    assert torch.equal(got[ended & ~arrived & torch.isfinite(shortest)], torch.zeros(int((ended & ~arrived & torch.isfinite(shortest)).sum())))
