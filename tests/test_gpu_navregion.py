"""Regions on the GPU (cuda.regions, Regions.labels_at / at / together / masks, SeenMaps.frontier_regions): the kernels are held to
EQUALITY with tests/test_navregion_host.py's region_rule, and to what the distance fields say by another road."""
import numpy as np
import pytest
import torch

from tests.test_navfield_host import CELL, RADIUS, F, bits, plans
from tests.test_navregion_host import region_rule, same, serpentine
from tests.test_gpu_navseen import _by_hand, _np, _odd_grid, _six

pytestmark = pytest.mark.gpu


def _result(r):
    return {k: _np(getattr(r, k)) for k in ('labels', 'areas', 'counts', 'open_cells', 'largest', 'largest_cells')}


def _rule(r, mask=None, before=None):
    """region_rule on a mirror of what the Regions ``r`` reads, as it stands."""
    grid = r.grid
    return region_rule.call(grid._host_geom, grid._host_starts, grid.cell, _np(grid.free), r.n_fields, _np(r.marks), r.where, _np(r.among),
                            _np(mask), before)


def _same(r, mask=None, before=None):
    want = _rule(r, mask, before)
    same(_result(r), want)
    return want


_WORLD = {}


def _world():
    """The six plans' grid, its regions (with passes) and the rule's, shared by the tests - and left unchanged."""
    if not _WORLD:
        from megastep_amd import cuda
        c = _six()['core']
        grid = cuda.nav_grid(c.scenery, clearance=RADIUS)
        r = cuda.regions(grid, passes=True)
        _WORLD.update(core=c, grid=grid, regions=r, want=_rule(r))
    return _WORLD


def test_regions_are_the_rules_on_the_six_plans():
    from megastep_amd import cuda
    w = _world()
    r = w['regions']
    same(_result(r), w['want'])
    assert isinstance(r, cuda.Regions) and r.n_fields == 1 and r.labels.dtype == torch.int32 and r.areas.dtype == torch.float32
    assert (r.passes >= 1).all() and (r.counts >= 1).all() and (r.largest_cells > 500).all()
    print('passes on the six plans:', _np(r.passes).reshape(-1).tolist())
    first, ny, nx = w['grid'].cells(2)
    assert r.image(2).shape == (ny, nx) and r.image(2).dtype == torch.int32 and r.area_image(2).shape == (ny, nx)
    assert torch.equal(r.image(2).reshape(-1), r.labels[first:first + ny*nx])
    assert torch.equal(r.image(2) >= 0, w['grid'].image(2)) and torch.equal(r.area_image(2) > 0, w['grid'].image(2))


@pytest.mark.parametrize('which', [0, 1, 2])
def test_every_lds_capacity_its_next_size_and_the_global_path(which):
    from megastep_amd import cuda
    capacity = cuda.REGION_CAPACITY[which]
    s = int(capacity**.5) - 2
    while (s + 3)**2 <= capacity:
        s += 1
    assert (s + 2)**2 <= capacity < (s + 3)**2
    rng = np.random.RandomState(which)
    small = ((1, -2, 9, 7), rng.rand(7, 9) < .7)
    for side in (s, s + 1):                          # (s + 1: the next instantiation; beyond the last: labelled in global memory)
        grid = _by_hand([((-3, 5, side, side), serpentine(side)), small])
        assert grid._max_framed == (side + 2)**2 and (grid._max_framed <= capacity) == (side == s)
        r = cuda.regions(grid, passes=True)
        want = _same(r)
        assert want['counts'][:, 0].tolist()[0] == 1 and want['largest_cells'][0, 0] == int(serpentine(side).sum()) and (r.passes >= 1).all()
        print('capacity', capacity, 'side', side, 'passes', _np(r.passes).reshape(-1).tolist())
    # two marked fields an env, a random mask of cells: many regions, both paths of the count
    marks = torch.as_tensor((rng.rand(2*grid.n_cells) < .6).astype(np.uint8), device='cuda')
    r = cuda.regions(grid, marks, 2, where=bool(which % 2), passes=True)
    want = _same(r)
    assert (want['counts'][0] > 50).all() and (r.passes >= 1).all()


def test_the_global_path_on_a_real_size_an_env_without_cells_and_marks():
    from megastep_amd import cuda
    grid = _odd_grid()
    assert grid._max_framed > cuda.REGION_CAPACITY[2] and grid.cells(3)[1]*grid.cells(3)[2] > 2**19
    r = cuda.regions(grid, passes=True)
    want = _same(r)
    assert want['counts'][:, 0].tolist() == [want['counts'][0, 0], 0, 1, 1] and want['largest'][:, 0].tolist() == [want['largest'][0, 0], -1, 0, 0]
    assert want['largest_cells'][3, 0] == 800*801 and _np(r.passes)[:, 0].tolist()[1] == 0 and (_np(r.passes)[[0, 2, 3], 0] >= 1).all()
    # marks that cut the large env into stripes and blobs
    rng = np.random.RandomState(8)
    image = rng.rand(801, 800) < .7
    image[::50] = False
    marks = np.ones(grid.n_cells, np.uint8)
    marks[grid.cells(3)[0]:grid.cells(3)[0] + 800*801] = image.reshape(-1)
    among = torch.as_tensor((rng.rand(grid.n_cells + 1) < .9).astype(np.uint8), device='cuda')
    r = cuda.regions(grid, torch.as_tensor(marks, device='cuda'), 1, among=among, passes=True)
    want = _same(r)
    assert want['counts'][3, 0] > 1000 and (_np(r.passes)[[0, 2, 3], 0] >= 1).all()
    print('passes on the odd grid:', _np(r.passes).reshape(-1).tolist())


def _spawn(w):
    return w['core'].agents.positions[:, :1].contiguous()


def test_the_mask_of_a_spawn_point_is_floorcoverages_reachable():
    from megastep_amd import cuda
    from megastep_amd.demo.envs.floorcoverage import reachable
    w = _world()
    grid, r = w['grid'], w['regions']
    layer = r.masks(points=_spawn(w))
    assert isinstance(layer, cuda.CellLayer) and layer.n_fields == 1 and layer.values.dtype == torch.uint8 and not layer.is_float
    want = reachable(grid, _spawn(w)[:, 0])
    assert torch.equal(layer.values[:grid.n_cells], want[:grid.n_cells]) and int(want.sum()) > 3000
    # the rule's masks, by points and by labels, two requests an env; out= is written in full
    points = w['core'].agents.positions.contiguous()
    out = r.masks(points=points)
    geom, starts = grid._host_geom, grid._host_starts
    assert np.array_equal(_np(out.values), region_rule.masks(geom, starts, CELL, w['want']['labels'], 1, points=_np(points)))
    wanted = torch.stack([r.largest[:, 0], torch.full_like(r.largest[:, 0], -1)], 1)
    out.values.fill_(7)
    assert r.masks(labels=wanted, out=out) is out
    assert np.array_equal(_np(out.values), region_rule.masks(geom, starts, CELL, w['want']['labels'], 1, wanted=_np(wanted)))
    with pytest.raises(RuntimeError, match='out'):
        r.masks(points=_spawn(w), out=out)
    largest = r.largest_mask()
    assert np.array_equal(_np(largest.values), region_rule.masks(geom, starts, CELL, w['want']['labels'], 1, wanted=_np(r.largest[:, :1])))
    assert torch.equal(largest.values[:grid.n_cells].long().sum().reshape(1), r.largest_cells.long().sum().reshape(1))
    # the layer as it is: an among, a countable mask
    assert cuda.seeded_fields(grid, grid.free, 1, among=largest.values).n_seeds.tolist() == r.largest_cells.tolist()
    assert cuda.seen_maps(grid, 1, countable=largest.values).n_countable.tolist() == r.largest_cells[:, 0].tolist()


def test_together_is_where_the_geodesic_is_finite_and_labels_at_is_the_rules():
    from megastep_amd import cuda
    w = _world()
    grid, r = w['grid'], w['regions']
    rng = np.random.RandomState(21)
    labels = w['want']['labels']
    a, b = np.empty((6, 32, 2), F), np.empty((6, 32, 2), F)
    for n in range(6):
        first, ny, nx = grid.cells(n)
        x, y = (_np(t) for t in grid.centres(n))
        store = labels[first:first + ny*nx]
        home = np.flatnonzero(store == w['want']['largest'][n, 0])
        others = np.flatnonzero((store >= 0) & (store != w['want']['largest'][n, 0]))
        for pts, cells in ((a, rng.choice(home, 32)), (b, np.concatenate([rng.choice(home, 16), rng.choice(others if len(others) else home, 16)]))):
            pts[n, :, 0], pts[n, :, 1] = x[cells % nx], y[cells//nx]
            pts[n] += rng.uniform(-.4, .4, (32, 2)).astype(F)*F(CELL)
    a[0, 0], b[1, 1] = np.nan, 1e9
    ta, tb = torch.as_tensor(a, device='cuda'), torch.as_tensor(b, device='cuda')
    found = r.labels_at(ta)
    assert found.shape == (6, 32, 4) and found.dtype == torch.int32
    assert np.array_equal(_np(found), region_rule.labels_at(grid._host_geom, grid._host_starts, CELL, labels, 1, a))
    assert np.array_equal(_np(r.at(ta)), region_rule.at(_np(found))) and (_np(found)[0, 0] == -1).all()
    together = r.together(ta, tb)
    assert together.dtype == torch.bool and torch.equal(together, torch.isfinite(cuda.geodesic(grid, ta, tb)))
    assert together.any() and (~together).any()
    assert np.array_equal(_np(together), region_rule.together(_np(found), _np(r.labels_at(tb))))
    field = torch.zeros((6, 32), dtype=torch.int64, device='cuda')
    field[3] = 1
    odd = r.labels_at(ta, field=field)
    assert torch.equal(odd[[0, 1, 2, 4, 5]], found[[0, 1, 2, 4, 5]]) and (odd[3] == -1).all()


def _marked(w, frames=1):
    from megastep_amd import cuda
    maps = cuda.seen_maps(w['grid'], 2)
    for frame in _six()['frames'][:frames]:
        maps.mark(*frame)
    return maps


def test_frontier_regions_are_the_frontier_fields_seeds():
    w = _world()
    maps = _marked(w)
    fields = maps.frontier_fields()
    r = maps.frontier_regions(passes=True)
    assert r.marks.data_ptr() == maps.values.data_ptr() and r.where is False and r.among.data_ptr() == maps.countable.data_ptr() and r.n_fields == 2
    assert torch.equal(r.open_cells, fields.n_seeds) and (r.open_cells > 0).all()
    n = 2*w['grid'].n_cells
    assert torch.equal(r.labels[:n] >= 0, fields.values[:n] == 0)
    want = _same(r)
    assert (want['counts'] > 1).any() and (r.passes >= 1).all()
    print('frontier passes after one frame:', _np(r.passes).reshape(-1).tolist())


def test_mask_out_update_a_side_stream_and_a_graph_replayed_three_times():
    from megastep_amd import cuda
    w = _world()
    grid = w['grid']
    frames = _six()['frames']
    maps = cuda.seen_maps(grid, 2)
    # a fresh call with a mask: the other fields have no open cell
    mask = torch.as_tensor(np.random.RandomState(6).rand(6, 2) < .5, device='cuda')
    mask[0, 0], mask[0, 1] = True, False
    r = maps.frontier_regions(mask=mask, passes=True)
    blank = dict(labels=np.full(2*grid.n_cells, -1, np.int32), areas=np.zeros(2*grid.n_cells, F), counts=np.zeros((6, 2), np.int32),
                 open_cells=np.zeros((6, 2), np.int32), largest=np.full((6, 2), -1, np.int32), largest_cells=np.zeros((6, 2), np.int32))
    first = _same(r, mask, blank)
    assert (_np(r.passes)[~_np(mask)] == 0).all() and (_np(r.passes)[_np(mask)] >= 1).all() and first['counts'][0].tolist() == [first['counts'][0, 0], 0]
    # update(mask) in place after a frame: the masked-out fields keep what they held
    tensors = (r.labels, r.areas, r.counts, r.open_cells, r.largest, r.largest_cells, r.passes)
    maps.mark(*frames[0])
    assert r.update(~mask) is r
    second = _same(r, ~mask, first)
    assert not np.array_equal(second['labels'], first['labels'])
    # out=: the same tensors; another grid, other marks or other arguments are refused
    maps.mark(*frames[1])
    got = maps.frontier_regions(mask=mask, out=r)
    assert got is r and all(x is y for x, y in zip(tensors, (r.labels, r.areas, r.counts, r.open_cells, r.largest, r.largest_cells, r.passes)))
    third = _same(r, mask, second)
    for kw in (dict(marks=maps.values.clone()), dict(where=True), dict(among=None), dict(n_fields=1, marks=maps.values[:grid.n_cells])):
        with pytest.raises(RuntimeError, match='`out` must come from a regions call'):
            cuda.regions(grid, **{**dict(marks=maps.values, n_fields=2, where=False, among=maps.countable), **kw}, out=r)
    # a side stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        r.update()
    side.synchronize()
    _same(r)
    # captured once, replayed three times, the maps marked in between: each replay is the rule on the maps as they stood
    maps.values.zero_()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        r.update()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        r.update()
    seen = []
    for replay in range(3):
        if replay:
            maps.mark(*frames[replay - 1])
        graph.replay()
        seen.append(_same(r)['open_cells'].copy())
    assert (seen[0] > seen[1]).all() and (seen[1] >= seen[2]).all() and (seen[1] > seen[2]).any()


def test_draws_gated_by_the_largest_region_and_in_a_band_of_areas():
    from megastep_amd import cuda
    w = _world()
    grid, r = w['grid'], w['regions']
    starts = torch.as_tensor(grid._host_starts[:-1], device='cuda')[:, None, None]
    draws = cuda.cell_draws(grid, grid, 2, 64, gate=r.largest_mask(), seed=5)
    assert (draws.counts == r.largest_cells).all() and (draws.cells >= 0).all()
    assert torch.equal(r.labels[(starts + draws.cells).reshape(-1)].reshape(6, 2, 64), r.largest[:, :, None].expand(6, 2, 64).contiguous())
    # a band of areas that begins between two region areas of a plan
    sizes = np.unique(np.concatenate([np.unique(w['want']['areas'][grid.cells(n)[0]:grid.cells(n)[0] + grid.cells(n)[1]*grid.cells(n)[2]]) for n in range(6)]))
    sizes = sizes[sizes > 0]
    assert len(sizes) >= 2, 'these plans have one region each'
    lo = float((sizes[-2].astype(np.float64) + sizes[-1])/2)
    draws = cuda.cell_draws(grid, r, 1, 64, lo=lo, hi=float('inf'), seed=6)
    drawn = draws.cells >= 0
    assert drawn.any() and torch.equal(drawn.all(-1), draws.counts > 0)
    at = (starts + draws.cells.clamp(min=0)).reshape(-1)
    assert torch.equal(draws.values[drawn], r.areas[at].reshape(6, 1, 64)[drawn]) and (draws.values[drawn] >= lo).all()
    every = cuda.cell_draws(grid, r, 1, 64, lo=float(sizes[0]), hi=float('inf'), seed=6)
    assert torch.equal(every.counts, r.open_cells)


def test_a_map_channel_of_the_areas_is_the_window_rule_on_them():
    from megastep_amd import cuda
    from tests.test_gpu_navwindow import _same as same_window
    w = _world()
    grid, r = w['grid'], w['regions']
    scale = 1./float(r.areas.max())
    views = cuda.agent_views(w['core'].agents, 16, 3.)
    got = _np(same_window(grid, views, 16, [cuda.map_channel(r, scale=scale), cuda.map_channel(r, scale=4*scale, gate=r.largest_mask(), hidden=.5)]))
    assert ((got[:, :, 0] > 0) & (got[:, :, 0] <= 1)).any() and (got[:, :, 0] == 0).any() and (got[:, :, 1] == F(.5)).any()
    assert cuda.cell_layer(r).values is r.areas and cuda.cell_layer(r).n_fields == 1


def test_sampled_spawns_gated_by_the_largest_region():
    from megastep_amd import cuda, modules
    w = _world()
    c, grid, r = w['core'], w['grid'], w['regions']
    plain = modules.SampledSpawns(c, grid, seed=7)
    gated = modules.SampledSpawns(c, grid, seed=7, gate=r.largest_mask())
    everyone = c.agent_full(True)
    for trial in range(3):
        request = gated.draw(everyone)
        assert torch.equal(gated.draws.counts, r.largest_cells.expand(6, 2)) and request['mask'].all()
        assert torch.equal(r.at(request['positions'][:, :, 0].contiguous()), r.largest.expand(6, 2))
    plain.draw(everyone)
    assert torch.equal(plain.draws.counts, r.open_cells.expand(6, 2)) and plain.draws.gate is None


class _Expert:
    """An env whose step is the expert's: the decision handed in is ignored."""

    def __init__(self, env):
        self.env = env

    def __getattr__(self, name):
        return getattr(self.env, name)

    def step(self, decision):
        return self.env.step(self.env.expert())


@pytest.mark.parametrize('graphed', [False, True])
def test_pointgoal_in_one_region(graphed):
    from megastep_amd import arrdict, cuda, graphs, modules
    from megastep_amd.demo import PointGoal
    geoms = plans(8)
    torch.manual_seed(4); np.random.seed(4)
    env = PointGoal(8, n_agents=2, geometries=geoms, goal_range=(1., 4.), sampled_spawns=True, one_region=True)
    r = env.regions
    assert isinstance(r, cuda.Regions) and r.grid is env.grid and env._respawner._gate is not None
    stepper = graphs.GraphedStep(_Expert(env), warmup=3) if graphed else _Expert(env)
    stepper.reset()
    nothing = arrdict.arrdict(actions=torch.zeros((8, 2), dtype=torch.long, device='cuda'))
    for t in range(10):
        if t:
            stepper.step(nothing)
        # the band is not empty on these plans: what follows is about connectivity, not about the band's width
        assert (env._goals.draws.counts > 0).all()
        assert torch.equal(r.at(env.core.agents.positions.contiguous()), r.largest.expand(8, 2))
        assert not env._goals.stranded.any()
    assert torch.equal(env._respawner.draws.counts, r.largest_cells.expand(8, 2))
    # without one_region the env builds and steps as before
    torch.manual_seed(4); np.random.seed(4)
    plain = PointGoal(8, n_agents=2, geometries=geoms, goal_range=(1., 4.), sampled_spawns=True)
    assert plain.regions is None and plain._respawner._gate is None and isinstance(plain._respawner, modules.SampledSpawns)
    plain.reset()
    world = plain.step(plain.expert())
    assert world.reward.shape == (8, 2) and torch.isfinite(world.reward).all() and plain._respawner.draws.gate is None
    with pytest.raises(RuntimeError, match='sampled_spawns'):
        PointGoal(8, geometries=geoms, one_region=True)
