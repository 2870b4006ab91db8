"""Cell draws on the GPU: `cuda.cell_draws` equal to the numpy statement of the contract (tests/test_navdraw_host.draw_rule) - cells,
points, uniforms, values, counts and the counter, exactly - on a band of a real distance field, on the free cells alone and on a
real seen map behind a gate; a plan whose bitmap exceeds 64 KiB of LDS, an env without cells and a band nothing falls in; masks,
`out=`, `again()`, streams and graph capture; `modules.SampledGoals`, `modules.SampledSpawns`; and `PointGoal` with both, eager
and as one HIP graph."""
import numpy as np
import pytest
import torch

from tests.test_navfield_host import CELL, RADIUS, F, plans
from tests.test_navdraw_host import draw_rule, same
from tests.test_navwindow_host import Layer
from tests.test_gpu_navseen import _np, _odd_grid, _six

pytestmark = pytest.mark.gpu


def _mirror(layer):
    return None if layer is None else Layer(_np(layer.values), layer.n_fields, _np(layer.field))


def _result(draws):
    return {k: _np(getattr(draws, k)) for k in ('cells', 'points', 'uniforms', 'values', 'counts', 'counter')}


def _rule(draws, counter, mask=None, before=None):
    """What the rule makes of the call that `draws` holds the arguments of, from `counter` on."""
    grid = draws.grid
    return draw_rule.call(grid._host_geom, grid._host_starts, grid.cell, _np(grid.free), _mirror(draws.source), draws.n_sets, draws.n_draws,
                          counter, lo=draws.lo, hi=draws.hi, where=draws.where, gate=_mirror(draws.gate), seed=draws.seed,
                          mask=None if mask is None else _np(mask), before=before)


def _same(grid, source, P, K, **kw):
    from megastep_amd import cuda
    draws = cuda.cell_draws(grid, source, P, K, **kw)
    want = _rule(draws, np.zeros((grid.n_envs, P), np.int32))
    same(_result(draws), want)
    assert draws.cells.dtype == torch.int32 and draws.points.shape == (grid.n_envs, P, K, 2) and (want['counter'] == 1).all()
    return draws, want


_WORLD = []


def _world():
    """The six plans' grid, the distance fields round agent 0, two seen maps an env after one marked render frame, and the cells
    agent 0 can walk to as a gate: (core, grid, fields, maps, reach)."""
    if not _WORLD:
        from megastep_amd import cuda
        w = _six()
        c = w['core']
        grid = cuda.nav_grid(c.scenery, clearance=RADIUS)
        assert grid.cell == CELL
        fields = cuda.distance_fields(grid, c.agents.positions[:, :1].contiguous())
        maps = cuda.seen_maps(grid, 2)
        maps.mark(*w['frames'][0])
        reach = torch.isfinite(fields.values).to(torch.uint8)
        _WORLD.append((c, grid, fields, maps, reach))
    return _WORLD[0]


@pytest.mark.parametrize('K', [1, 7, 256])
def test_draws_are_the_rules_on_the_six_plans(K):
    c, grid, fields, maps, reach = _world()
    draws, want = _same(grid, fields, 2, K, lo=1., hi=4., seed=K)
    assert (want['counts'] > 100).all() and (want['values'] >= 1).all() and (want['values'] <= 4).all()
    at = grid._host_starts[:-1, None, None] + want['cells']
    assert (_np(grid.free)[at] != 0).all() and np.array_equal(_np(fields.values)[at], want['values'])
    assert K == 1 or not np.array_equal(want['cells'][:, 0], want['cells'][:, 1])
    draws, want = _same(grid, grid, 2, K, seed=2**40 + 7)
    assert np.array_equal(want['counts'][:, 0], [int(grid.image(e).sum()) for e in range(6)]) and draws.values is None
    draws, want = _same(grid, maps, 2, K, where=False, gate=reach, seed=5)
    assert (want['counts'] > 100).all() and (want['counts'][:, 0] != want['counts'][:, 1]).any()
    for e in range(6):
        first, ny, nx = grid.cells(e)
        for s in range(2):
            assert not _np(maps.image(e, s)).reshape(-1)[want['cells'][e, s]].any() and _np(reach)[first + want['cells'][e, s]].all()


def test_a_bitmap_of_more_than_64_kib_an_env_without_cells_and_an_empty_band():
    grid = _odd_grid()
    assert grid.cells(3)[1]*grid.cells(3)[2] > 64*1024*8                                   # (more bits than 64 KiB of LDS)
    rng = np.random.RandomState(13)
    D = rng.uniform(0., 10., 3*grid.n_cells).astype(F)
    D[::11], D[3::13] = np.inf, np.nan
    D = torch.as_tensor(D, device='cuda')
    for K in (1, 256):
        draws, want = _same(grid, D, 3, K, lo=2., hi=2.5, seed=K)
        assert (want['counts'][1] == 0).all() and (want['cells'][1] == -1).all() and np.isnan(want['points'][1]).all() and np.isnan(want['values'][1]).all()
        assert (want['counts'][3] > 10000).all() and (want['cells'][[0, 2, 3]] >= 0).all()
    assert want['cells'][3].max() > 600000 and want['cells'][3].min() < 40000              # (the last lanes' spans and the first's)
    draws, want = _same(grid, grid, 1, 256)
    assert want['counts'][:, 0].tolist() == [int(grid.image(e).sum()) if grid.cells(e)[1] else 0 for e in range(4)]
    # a band nothing falls in
    draws, want = _same(grid, D, 3, 7, lo=20., hi=30.)
    assert (want['counts'] == 0).all() and (want['cells'] == -1).all() and np.isnan(want['points']).all() and np.isnan(want['values']).all()
    assert ((want['uniforms'] >= 0) & (want['uniforms'] < 1)).all()


@pytest.mark.parametrize('K', [1, 7, 256])
def test_the_hand_made_grids_of_the_cpu_suite(K):
    """1 x 1, 3 x 5, 65 cells, 64*256 + 1 cells, only the last cell free, none, all, no cells, 64 cells: one grid."""
    from megastep_amd import cuda
    from tests.test_navdraw_host import hand
    w = hand()
    dev = lambda a: torch.as_tensor(a, device='cuda')
    grid = cuda.NavGrid(dev(w.geom), dev(w.starts), dev(w.free), CELL, RADIUS, w.geom, w.starts)
    draws, want = _same(grid, grid, 2, K, seed=K)
    assert want['counts'][[4, 5, 6, 7], 0].tolist() == [1, 0, 81, 0] and (want['cells'][4] == 69).all()
    rng = np.random.RandomState(17)
    lo, hi = F(1.1), F(2.7)
    D = rng.uniform(0., 4., 2*w.n_cells).astype(F)
    D[::7], D[1::7], D[2::7], D[3::11] = lo, hi, np.nan, np.inf
    marks = rng.randint(0, 2, 3*w.n_cells).astype(np.uint8)
    field = rng.randint(-1, 4, (w.N, 2))                                                    # (-1 and 3: no store of three)
    field[3] = [2, 0]
    draws, want = _same(grid, cuda.cell_layer(dev(D), 2), 2, K, lo=float(lo), hi=float(hi), gate=cuda.cell_layer(dev(marks), 3, field=dev(field)), seed=9)
    assert (want['counts'][3] > 1000).all() and (K < 7 or ((want['values'] == lo).any() and (want['values'] == hi).any()))


def test_mask_out_again_a_side_stream_and_a_graph_replayed_three_times():
    from megastep_amd import cuda
    c, grid, fields, maps, reach = _world()
    rng = np.random.RandomState(4)
    draws, first = _same(grid, fields, 2, 7, lo=1., hi=4., seed=11)
    # a mask: the counter moves only where a set was computed
    mask = torch.as_tensor(rng.rand(6, 2) < .5, device='cuda')
    mask[0, 0], mask[0, 1] = True, False
    assert draws.again(mask=mask) is draws
    second = _rule(draws, first['counter'], mask, first)
    same(_result(draws), second)
    assert np.array_equal(second['counter'], 1 + _np(mask)) and np.array_equal(second['cells'][~_np(mask)], first['cells'][~_np(mask)])
    assert not np.array_equal(second['cells'][0, 0], first['cells'][0, 0])
    # out=: the same tensors, other arguments, the counter goes on
    tensors = (draws.cells, draws.points, draws.uniforms, draws.values, draws.counts, draws.counter)
    got = cuda.cell_draws(grid, fields, 2, 7, lo=2., hi=3., seed=12, mask=~mask, out=draws)
    assert got is draws and all(a is b for a, b in zip(tensors, (got.cells, got.points, got.uniforms, got.values, got.counts, got.counter)))
    third = _rule(draws, second['counter'], ~mask, second)
    same(_result(draws), third)
    assert (third['counter'] == 2).all()
    with pytest.raises(RuntimeError, match='out'):
        cuda.cell_draws(grid, fields, 2, 8, lo=2., hi=3., out=draws)
    with pytest.raises(RuntimeError, match='out'):
        cuda.cell_draws(grid, grid, 2, 7, out=draws)
    # a fresh call with a mask leaves the other sets blank
    fresh = cuda.cell_draws(grid, grid, 2, 7, mask=mask)
    blank = ~_np(mask)
    assert (_np(fresh.cells)[blank] == -1).all() and np.isnan(_np(fresh.points)[blank]).all() and (_np(fresh.counts)[blank] == 0).all()
    assert np.array_equal(_np(fresh.counter), _np(mask).astype(np.int32))
    # a side stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        draws.again()
    side.synchronize()
    fourth = _rule(draws, third['counter'])
    same(_result(draws), fourth)
    # captured once, replayed three times: each replay draws at the counter it finds
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        draws.again()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    counter = _np(draws.counter).copy()
    assert (counter == 4).all()
    with torch.cuda.graph(graph):
        draws.again()
    assert np.array_equal(_np(draws.counter), counter)                                     # (a capture runs nothing)
    seen = []
    for replay in range(3):
        graph.replay()
        want = _rule(draws, counter)
        same(_result(draws), want)
        counter = want['counter']
        seen.append(want['cells'].copy())
    assert (counter == 7).all() and not any(np.array_equal(a, b) for a, b in ((seen[0], seen[1]), (seen[1], seen[2]), (seen[0], seen[2])))


def test_sampled_goals_lie_in_the_band_from_where_the_agent_stands():
    from megastep_amd import modules
    c, grid = _world()[:2]
    everyone = c.agent_full(True)
    margin = CELL*2**.5
    for lo, hi in ((1., 3.), (2., 6.), (50., 60.)):
        goals = modules.SampledGoals(c, grid, lo, hi, seed=3)
        assert goals(everyone) is goals.goals and goals.goals.shape == (6, 2, 2)
        counts = goals.draws.counts
        assert torch.equal(goals.stranded, counts == 0) and bool(goals.stranded.all()) == (lo == 50.)
        far = goals.fields.at(c.agents.positions)
        assert torch.equal(far, goals.distances())
        ok = ~goals.stranded
        assert torch.isfinite(far[ok]).all() and (far[ok] >= lo - margin).all() and (far[ok] <= hi + margin).all()
        assert torch.equal(goals.goals[goals.stranded], c.agents.positions[goals.stranded])
        assert goals.observation().shape == (6, 2, 3) and goals.waypoints().shape == (6, 2, 2) and goals.space.shape == (2, 3)
        assert set(goals.state(1)) == {'goals', 'stranded'}
    # a masked draw moves the marked agents' goals only, and draws another cell
    goals = modules.SampledGoals(c, grid, 1., 6.)
    before = goals(everyone).clone()
    some = torch.as_tensor(np.random.RandomState(2).rand(6, 2) < .5, device='cuda')
    some[0, 0], some[0, 1] = True, False
    after = goals(some)
    assert torch.equal(after[~some], before[~some]) and not torch.equal(after[some], before[some])
    assert torch.equal(goals.draws.counter, 1 + some.int())
    follower = modules.PathFollower(c, goals)
    assert follower().actions.shape == (6, 2)
    with pytest.raises(RuntimeError, match='band'):
        modules.SampledGoals(c, grid, 3., 1.)


def test_sampled_spawns_stand_on_free_cells():
    from megastep_amd import cuda, modules
    c, grid, fields = _world()[:3]
    positions, angles = c.agents.positions.clone(), c.agents.angles.clone()
    try:
        for within in (None, fields):
            spawns = modules.SampledSpawns(c, grid, seed=7, within=within)
            seen = []
            for trial in range(3):
                reset = torch.as_tensor(np.random.RandomState(trial).rand(6, 2) < .7, device='cuda')
                request = spawns.draw(reset)
                assert request['positions'].shape == (6, 2, 1, 2) and request['angles'].shape == (6, 2, 1) and not request['choices'].any()
                assert torch.equal(request['mask'], reset) and request['after'] is False
                cells = _np(spawns.draws.cells)[..., 0]
                for e in range(6):
                    first, ny, nx = grid.cells(e)
                    x, y = (_np(t) for t in grid.centres(e))
                    for a in range(2):
                        if cells[e, a] >= 0:
                            assert _np(grid.free)[first + cells[e, a]] != 0
                            assert np.array_equal(_np(request['positions'])[e, a, 0], [x[cells[e, a] % nx], y[cells[e, a]//nx]])
                            assert within is None or np.isfinite(_np(fields.values)[first + cells[e, a]])
                heading = request['angles'][reset]
                assert (heading >= -180).all() and (heading < 180).all()
                assert torch.equal(request['angles'][..., 0], spawns.draws.uniforms[..., 0]*360. - 180.)
                seen.append(cells.copy())
            assert not np.array_equal(seen[0], seen[2])
            spawns(c.agent_full(True))
            assert torch.equal(c.agents.positions, spawns.draws.points[:, :, 0]) and not c.agents.velocity.any()
            assert (cuda.distance_fields(grid, c.agents.positions).at(c.agents.positions) < CELL*2).all()      # (somewhere an agent can walk from)
    finally:
        c.agents.positions[:] = positions
        c.agents.angles[:] = angles


class _Expert:
    """An env whose step is the expert's: the decision handed in is ignored."""

    def __init__(self, env):
        self.env = env

    def __getattr__(self, name):
        return getattr(self.env, name)

    def step(self, decision):
        return self.env.step(self.env.expert())


@pytest.mark.parametrize('graphed', [False, True])
def test_pointgoal_with_sampled_goals_and_spawns(graphed):
    from megastep_amd import arrdict, graphs, modules
    from megastep_amd.demo import PointGoal
    geoms = plans(6)
    torch.manual_seed(3); np.random.seed(3)
    plain = PointGoal(6, geometries=geoms, max_lifespan=30)
    want = plain.reset()
    torch.manual_seed(3); np.random.seed(3)
    env = PointGoal(6, geometries=geoms, max_lifespan=30, goal_range=(1., 4.), sampled_spawns=True)
    assert isinstance(env._goals, modules.SampledGoals) and isinstance(env._respawner, modules.SampledSpawns)
    stepper = graphs.GraphedStep(_Expert(env), warmup=3) if graphed else _Expert(env)
    world = stepper.reset()
    counts = env._goals.draws.counts
    first, stranded = env._distance.clone(), env._goals.stranded
    # nobody is stranded on its first goal unless its band was empty (or it stands where the grid defines no distance)
    assert stranded[counts == 0].all() and not (stranded & (counts > 0) & torch.isfinite(first)).any() and not stranded.all()
    ok = torch.isfinite(first) & (counts > 0)
    assert (first[ok] >= 1. - CELL*2**.5).all() and (first[ok] <= 4. + CELL*2**.5).all()
    nothing = arrdict.arrdict(actions=torch.zeros((6, 1), dtype=torch.long, device='cuda'))
    resets = 0
    for t in range(20):
        world = stepper.step(nothing)
        for key in ('rgb', 'd', 'goal'):
            assert world.obs[key].shape == want.obs[key].shape and world.obs[key].dtype == want.obs[key].dtype
        assert world.reward.shape == want.reward.shape == (6, 1) and world.reset.shape == want.reset.shape and world.reset.dtype == torch.bool
        assert torch.isfinite(world.reward).all() and torch.isfinite(env.core.agents.positions).all()
        resets += int(world.reset.sum())
    assert resets > 0 and (env._respawner.draws.counter > 0).all()
    # the plain env is what it was: the same first world from the same seeds, whatever was built in between
    torch.manual_seed(3); np.random.seed(3)
    again = PointGoal(6, geometries=geoms, max_lifespan=30)
    assert isinstance(again._goals, modules.Goals) and isinstance(again._respawner, modules.RandomSpawns)
    world = again.reset()
    for got, ref in ((world.obs.rgb, want.obs.rgb), (world.obs.d, want.obs.d), (world.obs.goal, want.obs.goal), (world.reward, want.reward),
                     (again.core.agents.positions, plain.core.agents.positions), (again.core.agents.angles, plain.core.agents.angles),
                     (again._goals.goals, plain._goals.goals)):
        assert torch.equal(got, ref)
