"""The nav calls at cell widths that are no power of two, and at a clearance that is not the default: every other nav test runs
at a cell of 0.125 m, where a cell's centre, a point's cell, the diagonal weight, a ray's sample count and an area are all exact
in binary32, so a slip in any of them is invisible. Here each call runs once at each of tests/test_navfield_host.CELLS on one
small world - toys.box(), two plain and two oblique plans, two agents, 64 rays, one rendered frame marked - against the numpy
rule its own test module holds it to, by the same equality, with `cell` passed through."""
import time

import numpy as np
import pytest
import torch

from tests.test_navfield_host import CELLS, F, bits, nav_rule, plans
from tests.test_navbasin_host import point_mark_rule
from tests.test_navregion_host import region_rule
from tests.test_navview_host import CONE
from tests import test_gpu_navbasin as on_basins, test_gpu_navdraw as on_draws, test_gpu_navfield as on_fields, \
    test_gpu_navpath as on_paths, test_gpu_navregion as on_regions, test_gpu_navseed as on_seeds, test_gpu_navview as on_views, \
    test_gpu_navwindow as on_windows
from tests.test_gpu_navseen import _Mirror, _core, _frame, _np

pytestmark = pytest.mark.gpu

N = 5
_WORLDS = {}


def _world(cell, r):
    """The world at one (cell, clearance): core, plans, grid, the frame, two seen maps an env with the frame marked (and the
    rule's mirror of them, checked), the distance fields of two goals an env, shared by the tests and left unchanged."""
    if (cell, r) not in _WORLDS:
        from megastep_amd import cuda, toys
        geoms = [toys.box()] + plans(2) + plans(2, oblique=True)
        c = _core(geoms, 2, 64)
        grid = cuda.nav_grid(c.scenery, cell=cell, clearance=r)
        assert bits(np.array([grid.cell, grid.clearance])).tolist() == bits(np.array([cell, r])).tolist()
        frame = _frame(c)
        maps = cuda.seen_maps(grid, 2)
        mirror = _Mirror(maps, cell)
        gained = maps.mark(*frame, max_range=4.)
        want = mirror.mark(*frame, max_range=4.)
        rng = np.random.RandomState(31)
        goals = on_fields._draw_goals(geoms, 2, rng)
        fields = cuda.distance_fields(grid, torch.as_tensor(goals, device='cuda'))
        _WORLDS[cell, r] = dict(core=c, geoms=geoms, grid=grid, frame=frame, maps=maps, mirror=mirror, gained=gained, want_gained=want,
                                goals=goals, fields=fields)
    return _WORLDS[cell, r]


def _timed(began, what, cell):
    print(f'{what} at cell {cell}: {time.time() - began:.2f} s')


@pytest.mark.parametrize('cell,r', CELLS)
def test_the_grid_the_fields_and_the_queries(cell, r):
    """nav_grid's geometry and free bytes (at the last pair: a clearance of its own), distance_fields and at."""
    began = time.time()
    w = _world(cell, r)
    good = on_fields._check(w['core'].scenery, w['grid'], w['fields'], w['goals'], np.random.RandomState(32), n_points=32, cell=cell, clearance=r)
    assert good >= .9*2*N, good
    free = [int(w['grid'].image(e).sum()) for e in range(N)]
    assert all(0 < f < w['grid'].cells(e)[1]*w['grid'].cells(e)[2] for e, f in enumerate(free))
    _timed(began, 'grid, fields and queries', cell)


@pytest.mark.parametrize('cell,r', CELLS)
def test_seen_maps_and_the_coverage_area(cell, r):
    from megastep_amd import modules
    began = time.time()
    w = _world(cell, r)
    w['mirror'].check(w['maps'], w['gained'], w['want_gained'])
    assert (w['want_gained'] > 0).all() and w['want_gained'].sum() > 500
    c = w['core']
    cover = modules.Coverage(c, w['grid'], max_range=4.)
    area = cover(modules.render(c, fields=('distances',)))
    # the kernel's order, in binary32: the cells as a float, times the square of the cell
    want = w['want_gained'].astype(F)*(F(cell)*F(cell))
    assert area.shape == (N, 2) and area.dtype == torch.float32 and np.array_equal(bits(_np(area)), bits(want))
    _timed(began, 'seen maps and area', cell)


def _seeded(w):
    from megastep_amd import cuda
    return w['maps'].frontier_fields(passes=True), cuda.seeded_fields(w['grid'], w['maps'].values, 2, where=True, passes=True)


@pytest.mark.parametrize('cell,r', CELLS)
def test_seeded_fields_and_frontier_fields(cell, r):
    began = time.time()
    w = _world(cell, r)
    grid, maps = w['grid'], w['maps']
    frontier, seen = _seeded(w)
    rng = np.random.RandomState(33)
    points = on_paths._points(w['core'].scenery, w['geoms'], rng, spread=16, spawn=16)
    which = rng.randint(0, 2, points.shape[:2]).astype(np.int32)
    which[:, ::9] = [[-1, 2, 7, -2**31]]
    good = 0
    for got, where, among in ((frontier, 0, maps.countable), (seen, 1, None)):
        want, counts = on_seeds._rule_fields(grid, maps.values, 2, where, among, cell)
        assert np.array_equal(_np(got.n_seeds), counts), (_np(got.n_seeds), counts)
        on_seeds._fields_equal(grid, got, want)
        good += sum(counts[e, g] > 0 and np.isfinite(want[e][g]).sum() > 500 for e in range(N) for g in range(2))
        rule = on_seeds._queries_equal(grid, got, want, points, which, cell)
        assert np.isfinite(rule).sum() > .3*rule.size and np.isinf(rule[:, ::9]).all()
    assert good >= .9*4*N, good
    _timed(began, 'seeded fields', cell)


@pytest.mark.parametrize('cell,r', CELLS)
def test_waypoints_and_paths_on_both_kinds_of_field(cell, r):
    began = time.time()
    w = _world(cell, r)
    grid = w['grid']
    rng = np.random.RandomState(34)
    points = on_paths._points(w['core'].scenery, w['geoms'], rng, spread=16, spawn=16)
    which = rng.randint(0, 2, points.shape[:2]).astype(np.int32)
    pts, goal = torch.as_tensor(points, device='cuda'), torch.as_tensor(which, device='cuda')
    for fields, rule in ((w['fields'], on_paths._rule), (_seeded(w)[0], on_seeds._follow_rule)):
        way, hops = fields.waypoints(pts, goal=goal, hops=True)
        found = fields.paths(pts, goal=goal, max_points=32)
        want_way, want_hops = rule(grid, fields, points, which, lookahead=16, cell=cell)
        want_paths, want_counts = rule(grid, fields, points, which, max_points=32, cell=cell)
        assert on_paths._equal(hops, want_hops) and on_paths._equal(way, want_way)
        assert on_paths._equal(found.counts, want_counts) and on_paths._equal(found.points, want_paths)
        assert torch.equal(hops < 0, torch.isinf(fields.at(pts, goal=goal))) and torch.equal(hops < 0, found.counts == 0)
        spawned = want_hops[:, 16:]
        assert (spawned >= 0).sum() >= .8*spawned.size, (spawned >= 0).sum()
        assert (want_hops >= 2).any() and (want_counts == 0).any()
    _timed(began, 'waypoints and paths', cell)


@pytest.mark.parametrize('cell,r', CELLS)
def test_local_maps_with_one_and_two_samples(cell, r):
    from megastep_amd import cuda
    began = time.time()
    w = _world(cell, r)
    c, grid, maps = w['core'], w['grid'], w['maps']
    seen = cuda.cell_layer(maps)
    channels = [cuda.map_channel(grid, gate=seen), cuda.map_channel(grid, where=False, gate=seen), cuda.map_channel(seen),
                cuda.map_channel(cuda.cell_layer(_seeded(w)[0]), scale=.1),
                cuda.map_channel(w['fields'], scale=.05, gate=seen, hidden=.25, outside=.5)]
    for size, samples, radius in ((16, 1, 2.), ((13, 21), 2, 3.)):
        got = _np(on_windows._same(grid, cuda.agent_views(c.agents, size, radius), size, channels, samples))
        assert (got[:, :, 0].sum((1, 2, 3)) > 0).all() and ((got[:, :, 3] > 0) & (got[:, :, 3] < 1)).any()
    _timed(began, 'local maps', cell)


@pytest.mark.parametrize('cell,r', CELLS)
def test_cell_draws_on_a_band_of_a_field(cell, r):
    began = time.time()
    w = _world(cell, r)
    draws, want = on_draws._same(w['grid'], w['fields'], 2, 7, lo=1., hi=4., seed=7)
    assert (want['counts'] > 0).all() and (want['values'] >= 1).all() and (want['values'] <= 4).all()      # every set has cells to draw from
    x, y = (_np(t) for t in w['grid'].centres(1))
    nx = len(x)
    assert np.array_equal(bits(want['points'][1, 0, :, 0]), bits(x[want['cells'][1, 0] % nx]))             # (a point is its cell's centre)
    _timed(began, 'cell draws', cell)


@pytest.mark.parametrize('cell,r', CELLS)
def test_regions_their_areas_and_together(cell, r):
    from megastep_amd import cuda
    began = time.time()
    w = _world(cell, r)
    grid = w['grid']
    reg = cuda.regions(grid, passes=True)
    want = on_regions._same(reg)                                          # (labels, float areas, counts, the largest)
    assert (reg.passes >= 1).all() and (want['largest_cells'] > 500).all()
    areas = _np(reg.areas)[:grid.n_cells]
    assert np.array_equal(bits(areas.max(keepdims=True)), bits(np.array([want['largest_cells'].max()], F)*(F(cell)*F(cell))))
    rng = np.random.RandomState(36)
    a = on_paths._points(w['core'].scenery, w['geoms'], rng, spread=8, spawn=24)
    b = on_paths._points(w['core'].scenery, w['geoms'], rng, spread=8, spawn=24)
    a[0, 0], b[1, 1] = np.nan, 1e9
    ta, tb = torch.as_tensor(a, device='cuda'), torch.as_tensor(b, device='cuda')
    found = reg.labels_at(ta)
    assert np.array_equal(_np(found), region_rule.labels_at(grid._host_geom, grid._host_starts, cell, want['labels'], 1, a))
    assert np.array_equal(_np(reg.at(ta)), region_rule.at(_np(found)))
    together = reg.together(ta, tb)
    assert torch.equal(together, torch.isfinite(cuda.geodesic(grid, ta, tb))) and together.any() and (~together).any()
    assert np.array_equal(_np(together), region_rule.together(_np(found), _np(reg.labels_at(tb))))
    _timed(began, 'regions', cell)


@pytest.mark.parametrize('cell,r', CELLS)
def test_view_fields_with_and_without_a_cone(cell, r):
    from megastep_amd import cuda
    began = time.time()
    w = _world(cell, r)
    c, grid, maps = w['core'], w['grid'], w['maps']
    walls = on_views._walls(c.scenery)
    points = c.agents.positions.contiguous()
    heads = torch.as_tensor((np.random.RandomState(37).uniform(-1, 1, (N, 2, 2))*np.array([.5, 3.])[None, :, None]).astype(F), device='cuda')
    for R, kw in ((4., {}), (3., dict(headings=heads, fov=CONE))):
        v = cuda.view_fields(grid, c.scenery, points, R, unseen=maps, **kw)
        want = on_views._same(v, walls)
        # visible and hidden free cells in every case
        for e in range(N):
            first, ny, nx = grid.cells(e)
            free = _np(grid.image(e)).reshape(-1)
            for p in range(2):
                vis = want['values'][2*first + p*ny*nx:2*first + (p + 1)*ny*nx].astype(bool)
                assert (vis & free).any() and (~vis & free).any(), (e, p)
        assert (want['counts'] > 0).all() and 0 < want['gains'].sum() < want['counts'].sum()
        bare = cuda.view_fields(grid, c.scenery, points, R, unseen=maps, store=False, **kw)
        assert bare.values is None and np.array_equal(_np(bare.counts), want['counts']) and np.array_equal(_np(bare.gains), want['gains'])
    _timed(began, 'view fields', cell)


@pytest.mark.parametrize('cell,r', CELLS)
def test_point_marks_basins_and_their_query(cell, r):
    from megastep_amd import cuda
    began = time.time()
    w = _world(cell, r)
    grid = w['grid']
    points = w['core'].agents.positions.clone()
    seeds = cuda.point_marks(grid, points, n_fields=1)
    marks, ids = point_mark_rule.call(grid._host_geom, grid._host_starts, cell, _np(grid.free), _np(points))
    assert np.array_equal(_np(seeds.marks), marks) and np.array_equal(_np(seeds.ids), ids) and marks.sum() >= N
    near = cuda.seeded_fields(grid, seeds.marks, 1)
    own = cuda.basins(near, ids=seeds.ids, n_ids=2, passes=True)
    want = on_basins._same(own)
    assert np.array_equal(want['sizes'].sum(-1), want['reached']) and (want['reached'] > 500).all()
    print('territories, passes:', _np(own.passes).reshape(-1).tolist(), 'longest chains:', want['longest'].reshape(-1).tolist())
    rng = np.random.RandomState(38)
    spread = torch.as_tensor(on_paths._points(w['core'].scenery, w['geoms'], rng, spread=8, spawn=24), device='cuda')
    field = torch.zeros((N, 32), dtype=torch.int64, device='cuda')
    field[:, 5] = 1
    got = own.at(spread, goal=field)
    assert np.array_equal(_np(got), on_basins._at_rule(own, spread, field)) and (got >= 0).sum() > .5*got.numel() and (got[:, 5] == -1).all()
    # the frontier's basins, by the clusters of the frontier
    frontier = _seeded(w)[0]
    clusters = w['maps'].frontier_regions()
    on_regions._same(clusters)
    b = cuda.basins(frontier, ids=clusters.labels, n_ids=256, passes=True)
    on_basins._same(b)
    assert (b.reached > 500).all()
    _timed(began, 'point marks and basins', cell)
