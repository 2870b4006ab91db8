"""Basins on the GPU (cuda.point_marks, cuda.basins, Basins.at / masks / update, modules.Territories, Frontiers(territories=...),
FloorCoverage.expert('split')): the kernels are held to EQUALITY with tests/test_navbasin_host.py's basin_rule, point_mark_rule and
basin_query_rule - chains followed cell by cell on a mirror of what the kernels read."""
import math

import numpy as np
import pytest
import torch

from tests.test_navfield_host import CELL, RADIUS, F, plans
from tests.test_navbasin_host import INT_MAX, basin_query_rule, basin_rule, bound, point_mark_rule, same
from tests.test_navregion_host import serpentine
from tests.test_gpu_navseen import _by_hand, _np, _odd_grid, _six

pytestmark = pytest.mark.gpu


def _result(b):
    n, g = b.grid.n_envs, b.n_fields
    return dict(labels=_np(b.labels), sizes=_np(b.sizes) if b.sizes is not None else np.zeros((n, g, 0), np.int32), reached=_np(b.reached))


def _rule(b, mask=None, before=None):
    """basin_rule on a mirror of what the Basins ``b`` reads, as it stands (the successors by the table: these grids are large)."""
    grid = b.grid
    return basin_rule.call(grid._host_geom, grid._host_starts, grid.cell, _np(grid.free), _np(b.fields.values), b.n_fields, _np(b.ids), b.n_ids,
                           _np(mask), before, table=True)


def _blank(b):
    n, g = b.grid.n_envs, b.n_fields
    return dict(labels=np.full(max(g*b.grid.n_cells, 1), -1, np.int32), sizes=np.zeros((n, g, b.n_ids), np.int32), reached=np.zeros((n, g), np.int32))


def _same(b, mask=None, before=None):
    want = _rule(b, mask, before)
    same(_result(b), want)
    if b.passes is not None:
        passes = _np(b.passes)
        computed = np.ones_like(passes, bool) if mask is None else _np(mask).astype(bool)
        cells = np.array([[b.grid.cells(e)[1]*b.grid.cells(e)[2] > 0]*b.n_fields for e in range(b.grid.n_envs)])
        assert (passes[computed & cells] >= 1).all()
        assert all(passes[n, g] <= bound(want['longest'][n, g]) for n, g in zip(*np.nonzero(computed & cells)))
    return want


def _at_rule(b, points, goal=None):
    grid = b.grid
    return basin_query_rule.call(grid._host_geom, grid._host_starts, grid.cell, _np(grid.free), _np(b.fields.values), _np(b.labels), b.n_fields,
                                 _np(points), _np(goal))


_WORLD = {}


def _world():
    """The six plans' grid, a frontier field after one marked render with its clusters as ids, and a two-agent point-mark field -
    shared by the tests, and left unchanged."""
    if not _WORLD:
        from megastep_amd import cuda
        six = _six()
        c = six['core']
        grid = cuda.nav_grid(c.scenery, clearance=RADIUS)
        maps = cuda.seen_maps(grid, 2)
        maps.mark(*six['frames'][0])
        frontier = maps.frontier_fields()
        clusters = maps.frontier_regions()
        points = c.agents.positions.clone()
        seeds = cuda.point_marks(grid, points, n_fields=1)
        near = cuda.seeded_fields(grid, seeds.marks, 1)
        _WORLD.update(core=c, grid=grid, maps=maps, frontier=frontier, clusters=clusters, points=points, seeds=seeds, near=near,
                      own=cuda.basins(near, ids=seeds.ids, n_ids=2, passes=True))
    return _WORLD


def test_on_the_six_plans_the_frontier_clusters_and_the_agents_territories_are_the_rules():
    from megastep_amd import cuda
    w = _world()
    grid, points = w['grid'], w['points']
    # which frontier cluster is nearest to every cell
    b = cuda.basins(w['frontier'], ids=w['clusters'].labels, n_ids=256, passes=True)
    assert isinstance(b, cuda.Basins) and b.n_fields == 2 and b.labels.dtype == torch.int32 and b.sizes.shape == (6, 2, 256)
    want = _same(b)
    assert (b.reached > 1000).all() and (want['sizes'].sum(-1) <= want['reached']).all()
    print('frontier basins, passes:', _np(b.passes).reshape(-1).tolist(), 'longest chains:', want['longest'].reshape(-1).tolist())
    got = b.at(points)                                                  # (agent k asks field k)
    assert got.shape == (6, 2) and got.dtype == torch.int32 and np.array_equal(_np(got), _at_rule(b, points)) and (got >= 0).all()
    assert torch.equal(w['frontier'].basins(ids=w['clusters'].labels, n_ids=256).labels, b.labels)
    # a label is a label of the clusters: the regions field's own, at the seeds
    seeds = w['frontier'].values[:2*grid.n_cells] == 0
    assert torch.equal(b.labels[:2*grid.n_cells][seeds], w['clusters'].labels[:2*grid.n_cells][seeds])
    # whose agent is nearest: the point marks, then the territories
    seeds, own = w['seeds'], w['own']
    marks, ids = point_mark_rule.call(grid._host_geom, grid._host_starts, CELL, _np(grid.free), _np(points))
    assert np.array_equal(_np(seeds.marks), marks) and np.array_equal(_np(seeds.ids), ids) and seeds.ids.dtype == torch.int32
    want = _same(own)
    assert np.array_equal(want['sizes'].sum(-1), want['reached']) and (want['sizes'][:, 0, 0] > 50).all()      # (agent 0 stands on free floor)
    print('territories, passes:', _np(own.passes).reshape(-1).tolist(), 'longest chains:', want['longest'].reshape(-1).tolist())
    field = torch.zeros((6, 2), dtype=torch.int64, device='cuda')
    got = own.at(points)                                                # (one field: both agents ask it)
    assert np.array_equal(_np(got), _at_rule(own, points, field)) and torch.equal(got, own.at(points, goal=field))
    assert got[:, 0].tolist() == [0]*6 and set(got[:, 1].tolist()) <= {0, 1}
    first, ny, nx = grid.cells(2)
    assert own.image(2).shape == (ny, nx) and torch.equal(own.image(2).reshape(-1), own.labels[first:first + ny*nx])
    odd = points.clone()
    odd[0, 0], odd[1, 1] = float('nan'), 1e9
    field[2, 0], field[3, 1] = -1, 1
    got = own.at(odd, goal=field)
    assert np.array_equal(_np(got), _at_rule(own, odd, field)) and got[0, 0] == got[1, 1] == got[2, 0] == got[3, 1] == -1


def _corridor(side):
    """(side*side,) float32: a field on serpentine(side) that falls by a cell's width at every cell from the corridor's far end to
    its start, +inf beside it - what any field with one seed at cell (0, 0) looks like to a hop; and the corridor's cells."""
    order = []
    for r in range(0, side, 2):
        order += [r*side + c for c in (range(side) if (r//2) % 2 == 0 else range(side - 1, -1, -1))]
        if r + 1 < side:
            order.append((r + 1)*side + (side - 1 if (r + 1) % 4 == 1 else 0))
    assert sorted(order) == np.flatnonzero(serpentine(side).reshape(-1)).tolist()
    values = np.full(side*side, np.inf, F)
    values[order] = np.arange(len(order)).astype(F)*F(CELL)
    return values, len(order)


def _sides(capacity):
    """The side whose framed cells just fit the launch of this capacity, the side whose cells just fit the capacity, and the next
    of each."""
    launch = math.isqrt(capacity) - 2
    assert (launch + 2)**2 <= capacity < (launch + 3)**2
    cells = math.isqrt(capacity)
    return sorted({launch, launch + 1, cells, cells + 1})


@pytest.mark.parametrize('which', [0, 1, 2])
def test_every_lds_capacity_its_next_size_and_the_global_path(which):
    from megastep_amd import cuda
    capacity = cuda.BASIN_CAPACITY[which]
    rng = np.random.RandomState(which)
    small = ((1, -2, 9, 7), rng.rand(7, 9) < .8)
    for side in _sides(capacity):
        grid = _by_hand([((-3, 5, side, side), serpentine(side)), small])
        assert grid._max_framed == (side + 2)**2
        marks = (rng.rand(2*grid.n_cells) < .01).astype(np.uint8)       # (field 1 of each env: random seeds)
        marks[:side*side] = 0
        marks[0] = 1                                                    # (field 0 of the corridor: one seed at its start)
        marks[2*side*side + 5] = 1
        # field 0 of the corridor is written by hand - a hop reads the values as they stand - and the relaxation of a corridor
        # of 20 000 cells is not what this test is about
        computed = torch.tensor([[False, True], [True, True]], device='cuda')
        fields = cuda.seeded_fields(grid, torch.as_tensor(marks, device='cuda'), 2, mask=computed)
        values, corridor = _corridor(side)
        fields.values[:side*side] = torch.as_tensor(values, device='cuda')
        ids = torch.as_tensor(rng.randint(-1, 5, 2*grid.n_cells).astype(np.int32), device='cuda')
        b = cuda.basins(fields, passes=True)
        want = _same(b)
        assert corridor == int(serpentine(side).sum()) and want['reached'][0, 0] == corridor and want['longest'][0, 0] == corridor - 1
        print('capacity', capacity, 'side', side, 'passes', _np(b.passes).reshape(-1).tolist(), 'longest', want['longest'].reshape(-1).tolist())
        mask = torch.as_tensor(rng.rand(2, 2) < .6, device='cuda')
        mask[0, 1] = True
        b = cuda.basins(fields, ids=ids, n_ids=4, mask=mask, passes=True)
        _same(b, mask, _blank(b))
        assert (_np(b.passes)[~_np(mask)] == 0).all()


def test_the_global_path_on_a_real_size_and_an_env_without_cells():
    from megastep_amd import cuda
    grid = _odd_grid()
    assert grid.cells(3)[1]*grid.cells(3)[2] > cuda.BASIN_CAPACITY[2] and grid.cells(1)[1] == 0
    rng = np.random.RandomState(12)
    marks = (rng.rand(grid.n_cells) < .002).astype(np.uint8)
    marks[[grid.cells(2)[0], grid.cells(3)[0]]] = 1                      # (each of the two open envs has a seed for sure)
    marks = torch.as_tensor(marks, device='cuda')
    fields = cuda.seeded_fields(grid, marks, 1)
    ids = torch.as_tensor(rng.randint(0, 300, grid.n_cells).astype(np.int32), device='cuda')
    b = cuda.basins(fields, ids=ids, n_ids=256, passes=True)
    want = _same(b)
    assert want['reached'][:, 0].tolist() == [want['reached'][0, 0], 0, 31*33, 800*801] and _np(b.passes)[1, 0] == 0 and (want['sizes'][1] == 0).all()
    assert (want['sizes'][3].sum() < want['reached'][3, 0]).all()
    print('passes on the odd grid:', _np(b.passes).reshape(-1).tolist(), 'longest chains:', want['longest'].reshape(-1).tolist())
    plain = cuda.basins(fields, passes=True)
    _same(plain)
    points = torch.as_tensor(rng.uniform(-45, 45, (4, 64, 2)).astype(F), device='cuda')
    assert np.array_equal(_np(plain.at(points)), _at_rule(plain, points))
    assert (plain.at(points)[1] == -1).all() and (plain.at(points)[3] >= 0).sum() > 30


def test_stale_values_break_chains_and_the_call_returns():
    from megastep_amd import cuda
    w = _world()
    grid = w['grid']
    near = cuda.seeded_fields(grid, w['seeds'].marks, 1)
    rng = np.random.RandomState(31)
    finite = torch.nonzero(torch.isfinite(near.values[:grid.n_cells]) & (near.values[:grid.n_cells] > .5)).reshape(-1)
    chosen = finite[torch.as_tensor(rng.choice(len(finite), 240, replace=False), device='cuda')]
    stale = torch.tensor([float('nan'), float('-inf'), 1e-3, float('inf'), -0., 7.], device='cuda').repeat(40)
    near.values[chosen] = stale
    b = cuda.basins(near, ids=w['seeds'].ids, n_ids=2, passes=True)
    want = _same(b)
    clean = _np(w['own'].labels)
    assert ((want['labels'] == -1) & (clean >= 0)).sum() > 300           # (what drains into the breaks, not the edited cells alone)
    assert (want['reached'] > 500).all()


def test_masks_are_the_labels_byte_for_byte_and_the_territories_partition_the_reached_cells():
    from megastep_amd import cuda
    w = _world()
    grid, own = w['grid'], w['own']
    wanted = torch.arange(2, device='cuda').expand(6, 2)
    mine = own.masks(labels=wanted)
    assert isinstance(mine, cuda.CellLayer) and mine.n_fields == 2 and mine.values.dtype == torch.uint8
    total = 0
    for e in range(6):
        first, ny, nx = grid.cells(e)
        labels = own.labels[first:first + ny*nx]
        stores = [mine.values[2*first + k*ny*nx:2*first + (k + 1)*ny*nx] for k in range(2)]
        for k in range(2):
            assert torch.equal(stores[k], (labels == k).to(torch.uint8))
        assert torch.equal(stores[0] + stores[1], (labels >= 0).to(torch.uint8))      # (a partition of the reached cells)
        total += int(stores[0].sum()) + int(stores[1].sum())
    assert total == int(own.reached.sum()) == int(own.sizes.sum())
    # labels no cell holds, -1 and out=: every byte is written
    mine.values.fill_(7)
    odd = torch.tensor([[1, -1], [5, 0]]*3, device='cuda')
    assert own.masks(labels=odd, out=mine) is mine
    for e in range(6):
        first, ny, nx = grid.cells(e)
        labels = own.labels[first:first + ny*nx]
        for k in range(2):
            want = (labels == odd[e, k]) & (labels >= 0)
            assert torch.equal(mine.values[2*first + k*ny*nx:2*first + (k + 1)*ny*nx], want.to(torch.uint8))
    with pytest.raises(RuntimeError, match='out'):
        own.masks(labels=odd[:, :1], out=mine)
    # a territory as it is: the marks of a seeded field
    mine = own.masks(labels=wanted)
    assert cuda.seeded_fields(grid, mine.values, 2).n_seeds.tolist() == own.sizes[:, 0].tolist()


def test_update_follows_points_moved_in_place_and_update_with_a_mask():
    from megastep_amd import cuda
    w = _world()
    grid = w['grid']
    points = w['points'].clone()
    seeds = cuda.point_marks(grid, points, n_fields=1)
    near = cuda.seeded_fields(grid, seeds.marks, 1)
    own = cuda.basins(near, ids=seeds.ids, n_ids=2, passes=True)
    first = _same(own)
    points[:, 1] = w['core'].agents.positions[:, 0] + torch.tensor([-.4, .3], device='cuda')
    points[:, 0] = w['points'][:, 1]
    assert seeds.update() is seeds
    marks, ids = point_mark_rule.call(grid._host_geom, grid._host_starts, CELL, _np(grid.free), _np(points))
    assert np.array_equal(_np(seeds.marks), marks) and np.array_equal(_np(seeds.ids), ids)
    near.update()
    tensors = (own.labels, own.sizes, own.reached, own.passes)
    mask = torch.tensor([[True], [False], [True], [True], [False], [True]], device='cuda')
    assert own.update(mask) is own and all(x is y for x, y in zip(tensors, (own.labels, own.sizes, own.reached, own.passes)))
    second = _same(own, mask, first)
    assert not np.array_equal(second['labels'], first['labels'])
    assert cuda.basins(near, ids=seeds.ids, n_ids=2, out=own) is own
    third = _same(own)
    assert not np.array_equal(third['labels'], second['labels'])
    for kw in (dict(ids=seeds.ids.clone()), dict(n_ids=3), dict(ids=None)):
        with pytest.raises(RuntimeError, match='`out` must come from a basins call'):
            cuda.basins(near, **{**dict(ids=seeds.ids, n_ids=2), **kw}, out=own)
    # ids given per point, and a store per point
    named = cuda.point_marks(grid, points, n_fields=2, ids=torch.tensor([[7, 3]]*6, device='cuda'))
    marks, ids = point_mark_rule.call(grid._host_geom, grid._host_starts, CELL, _np(grid.free), _np(points), 2, np.array([[7, 3]]*6))
    assert np.array_equal(_np(named.marks), marks) and np.array_equal(_np(named.ids), ids) and set(ids[marks != 0].tolist()) == {3, 7}


def test_one_graph_of_marks_field_and_basins_replayed_twice_after_moving_the_agents():
    from megastep_amd import cuda
    w = _world()
    grid = w['grid']
    points = w['points'].clone()
    seeds = cuda.point_marks(grid, points, n_fields=1)
    near = cuda.seeded_fields(grid, seeds.marks, 1)
    own = cuda.basins(near, ids=seeds.ids, n_ids=2, passes=True)

    def chain():
        seeds.update(); near.update(); own.update()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chain()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                       # (three launches and two fills, one after the other: a linear graph)
        chain()
    moves = (torch.tensor([.5, -.25], device='cuda'), torch.tensor([-.75, .5], device='cuda'))
    seen = []
    for move in moves:
        points[:, 1] = w['points'][:, 1] + move
        graph.replay()
        torch.cuda.synchronize()
        got = {k: v.copy() for k, v in _result(own).items()}
        fresh = cuda.point_marks(grid, points, n_fields=1)
        eager = cuda.basins(cuda.seeded_fields(grid, fresh.marks, 1), ids=fresh.ids, n_ids=2)
        same(got, _result(eager))
        assert torch.equal(seeds.ids, fresh.ids) and torch.equal(seeds.marks, fresh.marks)
        seen.append(got['labels'])
    _same(own)
    assert not np.array_equal(seen[0], seen[1])


def test_floorcoverage_split_sends_every_agent_to_floor_of_its_own_territory():
    from megastep_amd import cuda, modules
    from megastep_amd.demo import FloorCoverage
    torch.manual_seed(5); np.random.seed(5)
    env = FloorCoverage(8, n_agents=2, geometries=plans(8), shared=True, max_lifespan=10**6)
    env.reset()
    grid = env.grid
    starts = torch.as_tensor(grid._host_starts[:-1], device='cuda')[:, None]
    agent = torch.arange(2, device='cuda').expand(8, 2)
    mine = apart = 0
    for t in range(20):
        decision = env.expert('split')
        assert decision.actions.shape == (8, 2) and decision.actions.dtype == torch.int64 and ((decision.actions >= 0) & (decision.actions < 7)).all()
        frontiers, territories = env._split, env.territories
        assert isinstance(territories, modules.Territories) and frontiers.territories is territories and frontiers.own.n_goals == 2
        here = env.core.agents.positions
        own_distance = frontiers.own.at(here)
        finite = torch.isfinite(own_distance)
        # the seed each agent's own field leads it to is a cell of its own territory - by the territories' labels - and unseen
        ends = cuda.basins(frontiers.own).at(here)                      # (n_env, n_agent): a cell index, -1 without a path
        assert torch.equal(ends >= 0, finite)
        holder = territories.basins.labels[(starts + ends.clamp(min=0)).reshape(-1)].reshape(8, 2)
        assert torch.equal(holder[finite], agent[finite])
        fresh = finite & frontiers.due.any(-1, keepdim=True)             # (computed at this call: from the map as it stands)
        assert (frontiers._unseen[(starts + ends.clamp(min=0)).reshape(-1)].reshape(8, 2)[fresh] == 1).all()
        way = frontiers.waypoints()
        shared = frontiers.fields.waypoints(here, goal=frontiers._field)
        assert torch.equal(torch.isnan(way).any(-1), torch.isnan(shared).any(-1) & ~finite)
        assert torch.equal(way[~finite].view(torch.int32), shared[~finite].view(torch.int32))
        both = finite.all(-1)
        mine += int(finite.sum())
        apart += int((ends[both][:, 0] != ends[both][:, 1]).sum())
        areas = territories.areas()
        assert areas.shape == (8, 2) and torch.equal(areas, territories.basins.sizes[:, 0].float()*torch.tensor(CELL, device='cuda')**2)
        assert torch.equal(territories.basins.sizes[:, 0].sum(-1), territories.basins.reached[:, 0])
        env.step(decision)
    print('agents with a field of their own, and envs whose two agents head for different cells, over 20 steps:', mine, apart)
    # at the first step alone every agent stands on free floor with next to nothing seen: its territory holds unseen floor
    assert mine > 8 and apart > 0, (mine, apart)
    # the env's other experts still run
    for kind in ('frontier', 'views'):
        actions = env.expert(kind).actions
        assert actions.shape == (8, 2) and ((actions >= 0) & (actions < 7)).all()
        env.step(env.expert('split'))
    with pytest.raises(RuntimeError, match='shared=True'):
        FloorCoverage(8, n_agents=2, geometries=plans(8)).expert('split')
