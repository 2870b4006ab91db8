"""Map windows on the GPU: `cuda.local_maps` equal to the numpy statement of the contract (tests/test_navwindow_host.window_rule),
as bits, on real seen maps, frontier fields and distance fields through `cuda.agent_views`; images of one pixel and of one row,
NaN views, an env without cells and field indices out of range; `out=`, streams and graph capture; `modules.LocalMap` and
`FloorCoverage(local_map=True)`, eager and as one HIP graph."""
import numpy as np
import pytest
import torch

from tests.test_navfield_host import CELL, RADIUS, F, bits, plans
from tests.test_navwindow_host import Channel, Layer, views_round, window_rule
from tests.test_gpu_navseen import _actions, _np, _odd_calls, _odd_grid, _six

pytestmark = pytest.mark.gpu


def _mirror(ch):
    """A cuda.MapChannel as the rule reads it."""
    layer = lambda l: None if l is None else Layer(_np(l.values), l.n_fields, _np(l.field))
    return Channel(layer(ch.source), ch.where, ch.scale, layer(ch.gate), ch.outside, ch.hidden)


def _rule(grid, views, size, channels, samples=1):
    from megastep_amd import cuda
    size = (size, size) if isinstance(size, int) else size
    channels = [ch if isinstance(ch, cuda.MapChannel) else cuda.map_channel(ch) for ch in channels]
    return window_rule.call(grid._host_geom, grid._host_starts, grid.cell, _np(views), size, [_mirror(ch) for ch in channels], samples)


def _same(grid, views, size, channels, samples=1, **kw):
    from megastep_amd import cuda
    got = cuda.local_maps(grid, views, size, channels, samples=samples, **kw)
    want = _rule(grid, views, size, channels, samples)
    assert got.shape == want.shape and got.dtype == torch.float32
    assert np.array_equal(bits(_np(got)), bits(want)), (int((bits(_np(got)) != bits(want)).sum()), size, samples)
    return got


_WORLDS = {}


def _world(shared):
    """The six plans' seen maps after two rendered frames (a map an agent, or one an env), their frontier fields, and the
    distance fields of agent 0's position: (core, grid, maps, slot, channels)."""
    if shared not in _WORLDS:
        from megastep_amd import cuda
        w = _six()
        c = w['core']
        grid = cuda.nav_grid(c.scenery, clearance=RADIUS)
        assert grid.cell == CELL
        maps = cuda.seen_maps(grid, 1 if shared else 2)
        slot = torch.zeros((6, 2), dtype=torch.int64, device='cuda') if shared else None
        for frame in w['frames']:
            maps.mark(*frame, slot=slot)
        frontier = maps.frontier_fields()
        goal = cuda.distance_fields(grid, c.agents.positions[:, :1].contiguous())
        seen = cuda.cell_layer(maps, field=slot)
        channels = [cuda.map_channel(grid, gate=seen), cuda.map_channel(grid, where=False, gate=seen), cuda.map_channel(seen),
                    cuda.map_channel(cuda.cell_layer(frontier, field=slot), scale=.1),
                    cuda.map_channel(goal, scale=.05, gate=seen, hidden=.25, outside=.5)]
        _WORLDS[shared] = (c, grid, maps, slot, channels)
    return _WORLDS[shared]


@pytest.mark.parametrize('shared', [False, True])
def test_local_maps_are_the_rules_bits_on_real_maps_and_fields(shared):
    from megastep_amd import cuda
    c, grid, maps, slot, channels = _world(shared)
    assert int(maps.totals.sum()) > 3000
    for size, samples, radius in ((16, 1, 2.), ((13, 21), 3, 3.), (64, 1, 40.)):
        got = _np(_same(grid, cuda.agent_views(c.agents, size, radius), size, channels, samples))
        assert (got[:, :, 0].sum((1, 2, 3)) > 0).all() and got[:, :, 1].sum() > 0             # floor in every window, walls in some
        assert np.array_equal(got[:, :, 0] + got[:, :, 1], got[:, :, 2]) or samples > 1
        assert ((got[:, :, 3] > 0) & (got[:, :, 3] < 1)).any() and ((got[:, :, 4] == F(.25)).any() or samples > 1)
        if radius > 10:
            assert (got[:, :, 4] == F(.5)).any() and (got[:, :, 2] == 0).any()               # the window leaves the grid


def test_one_pixel_one_row_nan_views_an_env_without_cells_and_bad_indices():
    from megastep_amd import cuda
    grid = _odd_grid()
    maps = cuda.seen_maps(grid, 2)
    origins, dirs, distances, slot, _, max_range = next(iter(_odd_calls()))
    maps.mark(origins, dirs, distances, slot=slot, max_range=max_range)
    assert int(maps.totals.sum()) > 100
    rng = np.random.RandomState(3)
    floats = rng.uniform(-1., 3., 3*grid.n_cells).astype(F)
    floats[::11], floats[3::13], floats[5::17] = np.inf, np.nan, 0.
    floats = torch.as_tensor(floats, device='cuda')
    field = torch.as_tensor(rng.randint(0, 2, (4, 3)), device='cuda')
    bad = rng.randint(-1, 3, (4, 3))                                                     # (-1 and 2: no store of two)
    bad[0, 0], bad[2, 1], bad[3, 2] = -1, 2, 0
    bad = torch.as_tensor(bad, device='cuda')
    channels = [grid, cuda.map_channel(grid, where=False, gate=cuda.cell_layer(maps, field=field), hidden=.25),
                cuda.map_channel(cuda.cell_layer(maps, field=bad), outside=.5), cuda.map_channel(floats, scale=.5, outside=.75),
                cuda.map_channel(cuda.cell_layer(floats, 3), scale=2., gate=cuda.cell_layer(maps, field=bad), hidden=.125),
                cuda.map_channel(cuda.cell_layer(floats[:2*grid.n_cells], 2, field=bad), scale=1.)]
    centres = _np(origins).astype(np.float64)
    some_floor = some_hidden = False
    for size, samples, angle, pixel in (((1, 1), 1, 0., CELL), ((1, 1), 4, 37., 2.), ((1, 70), 2, 90., CELL), ((70, 1), 1, 180.5, 3*CELL),
                                        ((16, 16), 3, 37., CELL), ((33, 17), 2, 200., 4.)):
        views = views_round(centres, size, angle, pixel)
        views[0, 1, 2] = np.nan
        views[2, 0] = [np.inf, 0, 0, 0, -np.inf, 1]
        views[3, 2, 5] = 3e38
        got = _np(_same(grid, torch.as_tensor(views, device='cuda'), size, channels, samples))
        assert (got[0, 1, 2] == F(.5)).all() and (got[1, :, 0] == 0).all() and (got[1, :, 3] == F(.75)).all()      # NaN: no cell; env 1: no cells
        some_floor, some_hidden = some_floor or bool((got[[0, 2, 3], :, 0] > 0).any()), some_hidden or bool((got[:, :, 1] == F(.25)).any())
    assert some_floor and some_hidden


def test_out_a_side_stream_and_a_graph_replayed_three_times():
    from megastep_amd import cuda
    c, grid, maps, slot, channels = _world(False)
    views = cuda.agent_views(c.agents, 16, 2.)
    first = _same(grid, views, 16, channels, 2)
    out = torch.full_like(first, -5.)
    assert cuda.local_maps(grid, views, 16, channels, samples=2, out=out) is out and torch.equal(out, first)
    with pytest.raises(RuntimeError, match='out'):
        cuda.local_maps(grid, views, 16, channels, samples=2, out=out[:, :, :4].contiguous())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        there = cuda.local_maps(grid, views, 16, channels, samples=2)
    side.synchronize()
    assert torch.equal(there, first)
    # captured once, replayed three times with the agents moved and the views rewritten in place
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        cuda.local_maps(grid, views, 16, channels, samples=2, out=torch.empty_like(out))
    torch.cuda.current_stream().wait_stream(side)
    with torch.cuda.graph(graph):
        got = cuda.local_maps(grid, views, 16, channels, samples=2, out=out)
    positions, angles = c.agents.positions.clone(), c.agents.angles.clone()
    rng = np.random.RandomState(2)
    try:
        for trial in range(3):
            c.agents.positions[:] = positions + torch.as_tensor(rng.uniform(-.5, .5, (6, 2, 2)).astype(F), device='cuda')
            c.agents.angles[:] = angles + 70.*(trial + 1)
            views.copy_(cuda.agent_views(c.agents, 16, 2.))
            graph.replay()
            eager = cuda.local_maps(grid, views, 16, channels, samples=2)
            assert torch.equal(got, eager) and not torch.equal(eager, first)
    finally:
        c.agents.positions[:] = positions
        c.agents.angles[:] = angles


@pytest.mark.parametrize('shared', [False, True])
def test_the_local_map_module_is_the_call_it_stands_for(shared):
    from megastep_amd import cuda, modules
    c = _six()['core']
    grid = cuda.nav_grid(c.scenery, clearance=RADIUS)
    cover = modules.Coverage(c, grid, max_range=4., shared=shared)
    cover(modules.render(c, fields=('distances',)))
    extra = cuda.map_channel(cuda.cell_layer(cover.maps.frontier_fields(), field=cover._slot), scale=.2)
    local = modules.LocalMap(c, cover, size=16, radius=2., channels=('floor', 'wall', 'seen', extra))
    got = local()
    seen = cuda.cell_layer(cover.maps, field=cover._slot)
    views = cuda.agent_views(c.agents, 16, 2.)
    want = cuda.local_maps(grid, views, 16, [cuda.map_channel(grid, gate=seen), cuda.map_channel(grid, where=False, gate=seen), seen, extra])
    assert torch.equal(got, want) and tuple(got.shape[1:]) == local.space.shape == (2, 4, 16, 16) and torch.equal(local.views(), views)
    assert torch.equal(got[:, :, 0] + got[:, :, 1], got[:, :, 2]) and got[:, :, 0].sum() > 100          # floor + wall is what was seen
    assert local() is got and torch.equal(local.state(2), got[2]) and local.state(2) is not got
    if shared:
        assert torch.equal(_same(grid, views, 16, local.channels)[:, :, 2], got[:, :, 2])
    plain = modules.LocalMap(c, cover)
    assert plain.space.shape == (2, 2, 32, 32) and plain().shape == (6, 2, 2, 32, 32)
    with pytest.raises(RuntimeError, match='named channel'):
        modules.LocalMap(c, cover, channels=('floor', 'ceiling'))


def test_floor_coverage_hands_the_policy_its_map_eager_and_as_a_hip_graph():
    from megastep_amd import arrdict, cuda, graphs
    from megastep_amd.demo import FloorCoverage
    rng = np.random.RandomState(8)
    acts = [_actions(rng, 8, 1) for _ in range(5)]
    logs = []
    for graphed in (False, True):
        torch.manual_seed(3); np.random.seed(3)
        env = FloorCoverage(8, geometries=plans(8), max_lifespan=10**6, complete=.05, local_map=True)
        assert set(env.obs_space) == {'rgb', 'd', 'coverage', 'map'} and env.obs_space['map'].shape == (1, 2, 32, 32)
        stepper = graphs.GraphedStep(env, warmup=3) if graphed else env
        world = stepper.reset()
        assert world.obs['map'].shape == (8, 1, 2, 32, 32)
        log = []
        # the graphed env's first step call is four steps under its actions: three of warm-up and the captured one
        for a in (acts if graphed else [acts[0]]*3 + acts):
            world = stepper.step(arrdict.arrdict(actions=a))
            seen = cuda.local_maps(env.grid, env._local.views(), 32, [env.maps])
            assert torch.equal(world.obs['map'][:, :, 0] + world.obs['map'][:, :, 1], seen[:, :, 0])
            log.append((world.obs['map'].clone(), world.reward.clone(), env.maps.totals.clone()))
        logs.append(log)
    eager, graphed = logs
    for k in range(5):
        for got, want in zip(graphed[k], eager[k + 3]):
            assert torch.equal(got, want), k
    assert all(float(m[:, :, 0].sum()) > 0 for m, _, _ in graphed) and not torch.equal(graphed[0][0], graphed[4][0])
    state = env.state(0)
    assert state['map'].shape == (1, 2, 32, 32)
    # without the option the env is what it was
    plain = FloorCoverage(8, geometries=plans(8))
    assert set(plain.obs_space) == {'rgb', 'd', 'coverage'} and set(plain.reset().obs) == {'rgb', 'd', 'coverage'} and plain._local is None
    assert set(plain.state(0)) == {'core', 'rgb', 'd', 'seen', 'fraction', 'lifespan'}
