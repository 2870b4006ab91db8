"""Zones on the GPU (cuda.zones, Regions.zones / Basins.zones, Zones.update, modules.Assignments, FloorCoverage.expert('assign')): the
kernel is held to EQUALITY with tests/test_navzone_host.py's zone_rule - loops over cells, a Python min over (value bits, cell) - on
a mirror of what the kernel reads, and Assignments.choose to its Python loop."""
import itertools

import numpy as np
import pytest
import torch

from tests.test_navfield_host import F, plans
from tests.test_navzone_host import (EMPTY, KEYS, SHAPES, choose_by_loop, choose_cases, direct_labels, hand, ranked_labels, same, some_marks,
                                     some_values, zone_rule)
from tests.test_gpu_navseen import _by_hand, _np

pytestmark = pytest.mark.gpu


def _result(z):
    return {k: _np(getattr(z, k)) for k in KEYS}


def _rule(z, mask=None, before=None):
    """zone_rule on a mirror of what the Zones ``z`` reads, as it stands."""
    grid = z.grid
    return zone_rule(grid._host_geom, grid._host_starts, grid.cell, _np(z.labels), z.n_labels, z.n_fields, z.K, z.ranked, _np(z.values), z.n_values,
                     _np(z.marks), z.n_marks, z.where, z.within_marks, _np(mask), before)


def _same(z, mask=None, before=None):
    want = _rule(z, mask, before)
    same(_result(z), want)
    return want


_GRID = []


def _hand_grid():
    if not _GRID:
        w = hand()
        _GRID.append(_by_hand([(tuple(int(v) for v in g), np.ones((ny, nx), bool)) for g, (nx, ny) in zip(w.geom, SHAPES)]))
    return _GRID[0]


def _dev(a):
    return torch.as_tensor(a, device='cuda')


def _layers(w, rng, ranked, K, L=1, V=1, M=1, n_roots=7):
    from megastep_amd import cuda
    labels = cuda.cell_layer(_dev(w.layer(ranked_labels(rng, n_roots) if ranked else direct_labels(rng, K), L)), L)
    values = cuda.cell_layer(_dev(w.layer(some_values(rng), V)), V)
    marks = cuda.cell_layer(_dev(w.layer(some_marks(rng), M)), M)
    return labels, values, marks


@pytest.mark.parametrize('ranked', [True, False])
@pytest.mark.parametrize('K', [1, 5, 256])
def test_the_hand_made_grids(ranked, K):
    """1 x 1 cells, envs without cells, rows of 63 .. 65 and 255 .. 257 cells, K = 1 and 256; where=False, within_marks on and off."""
    from megastep_amd import cuda
    w, grid = hand(), _hand_grid()
    rng = np.random.RandomState(K + ranked)
    labels, values, marks = _layers(w, rng, ranked, K)
    z = cuda.zones(labels, values=values, marks=marks, n_zones=K, ranked=ranked, grid=grid)
    assert isinstance(z, cuda.Zones) and z.cells.shape == (len(SHAPES), 1, K) and z.points.shape == (len(SHAPES), 1, K, 2) and z.ranked == ranked
    assert z.cells.dtype == z.nearest.dtype == z.roots.dtype == z.n_zones.dtype == torch.int32 and z.least.dtype == torch.float32
    got = _same(z)
    for n in EMPTY:
        assert not got['cells'][n].any() and np.isinf(got['least'][n]).all() and np.isnan(got['points'][n]).all() and got['n_zones'][n, 0] == 0
    assert got['cells'].sum() > 100 and np.isfinite(got['least']).any()
    assert torch.equal(z.areas(), z.cells.float()*torch.tensor(grid.cell, device='cuda')**2)
    for where, within in ((False, False), (True, True), (False, True)):
        _same(cuda.zones(labels, values=values, marks=marks, n_zones=K, where=where, within_marks=within, ranked=ranked, grid=grid))
    plain = cuda.zones(labels, n_zones=K, ranked=ranked, grid=grid)
    _same(plain)
    assert torch.equal(plain.marked, plain.cells) and torch.isinf(plain.least).all() and (plain.nearest == -1).all()


def test_roots_at_the_last_cell_one_more_root_than_zones_and_ties():
    from megastep_amd import cuda
    w, grid = hand(), _hand_grid()
    # the only root at the last cell, the values falling towards it
    labels = cuda.cell_layer(_dev(w.layer(lambda n, cells: np.full(cells, cells - 1, np.int32), 1)))
    values = cuda.cell_layer(_dev(w.layer(lambda n, cells: np.arange(cells, 0, -1).astype(F), 1)))
    got = _same(cuda.zones(labels, values=values, n_zones=3, ranked=True, grid=grid))
    for n, cells in enumerate(w.sizes):
        if cells:
            assert got['roots'][n, 0].tolist() == [cells - 1, -1, -1] and got['nearest'][n, 0, 0] == cells - 1 and got['cells'][n, 0, 0] == cells
    # every cell its own root: K and K + 1 roots at 256 and 257 cells; the 257th zone is counted in n_zones alone
    labels = cuda.cell_layer(_dev(w.layer(lambda n, cells: np.arange(cells, dtype=np.int32), 1)))
    got = _same(cuda.zones(labels, values=values, n_zones=256, ranked=True, grid=grid))
    assert got['n_zones'][:, 0].tolist() == w.sizes and got['cells'][8, 0].sum() == 256 == got['cells'][9, 0].sum()
    # equal values: the least index; and a zone none of whose values takes part
    labels = cuda.cell_layer(_dev(w.layer(lambda n, cells: (np.arange(cells) % 2).astype(np.int32), 1)))
    bad = np.array([np.inf, np.nan, -1., -0., -np.inf, -1e-45], F)
    def make(n, cells):
        v = np.resize(bad, cells)
        v[1::2] = .25
        return v
    got = _same(cuda.zones(labels, values=cuda.cell_layer(_dev(w.layer(make, 1))), n_zones=2, ranked=False, grid=grid))
    many = np.array(w.sizes) > 1
    assert (got['nearest'][many, 0, 1] == 1).all() and (got['nearest'][:, 0, 0] == -1).all() and np.isinf(got['least'][:, 0, 0]).all()


@pytest.mark.parametrize('L, V, M', [c for c in itertools.product((1, 3), repeat=3) if max(c) == 3])
def test_every_combination_of_store_counts_and_a_mask(L, V, M):
    from megastep_amd import cuda
    w, grid = hand(), _hand_grid()
    rng = np.random.RandomState(9*L + 3*V + M)
    for ranked in (True, False):
        labels, values, marks = _layers(w, rng, ranked, 6, L, V, M, n_roots=6)
        z = cuda.zones(labels, values=values, marks=marks, n_zones=6, ranked=ranked, grid=grid, within_marks=bool(M & 1))
        assert z.n_fields == 3
        first = _same(z)
        # update in place, a mask: the other fields keep what they held
        z.labels[:] = _dev(w.layer(ranked_labels(rng, 6) if ranked else direct_labels(rng, 6), L))
        mask = _dev(rng.rand(len(SHAPES), 3) < .5)
        tensors = [getattr(z, k) for k in KEYS]
        assert z.update(mask) is z and all(a is b for a, b in zip(tensors, [getattr(z, k) for k in KEYS]))
        second = _same(z, mask, first)
        assert not np.array_equal(second['cells'], first['cells'])
        # out=
        assert cuda.zones(labels, values=values, marks=marks, n_zones=6, ranked=ranked, grid=grid, within_marks=bool(M & 1), out=z) is z
        _same(z)
        with pytest.raises(RuntimeError, match='`out` must come from a zones call'):
            cuda.zones(labels, values=values, marks=marks, n_zones=7, ranked=ranked, grid=grid, within_marks=bool(M & 1), out=z)
    fresh = cuda.zones(labels, values=values, marks=marks, n_zones=6, ranked=False, grid=grid, mask=mask)
    blank = zone_rule(grid._host_geom, grid._host_starts, grid.cell, np.full(1, -1, np.int32), 1, 3, 6, False, mask=np.zeros((len(SHAPES), 3), bool))
    _same(fresh, mask, blank)


def test_one_env_of_300_by_300_cells():
    """Beyond every other nav kernel's LDS tier: this kernel's LDS does not grow with the env."""
    from megastep_amd import cuda
    grid = _by_hand([((-150, -150, 300, 300), np.ones((300, 300), bool))])
    assert grid.n_cells == 90000 > max(cuda.FIELD_CAPACITY + cuda.REGION_CAPACITY + cuda.BASIN_CAPACITY)
    rng = np.random.RandomState(300)
    labels = cuda.cell_layer(_dev(ranked_labels(rng, 200)(0, 90000)))
    values = cuda.cell_layer(_dev(np.concatenate([rng.randint(0, 50, 90000).astype(F)*F(.125), np.zeros(1, F)])))
    marks = cuda.cell_layer(_dev(some_marks(rng)(0, 90000)))
    for K in (64, 256):
        got = _same(cuda.zones(labels, values=values, marks=marks, n_zones=K, ranked=True, grid=grid, within_marks=True))
        assert got['n_zones'][0, 0] == 200 and (got['cells'][0, 0, :min(K, 200)] > 100).all() and (got['least'][0, 0, :min(K, 200)] < .5).all()
    got = _same(cuda.zones(cuda.cell_layer(_dev(direct_labels(rng, 256)(0, 90000))), values=values, n_zones=256, ranked=False, grid=grid))
    assert got['n_zones'][0, 0] == 256 and got['cells'].sum() > 80000


_WORLD = {}


def _world():
    """FloorCoverage's world on 8 plans, two agents sharing a map, after the reset's one rendered, marked frame: the grid's regions,
    the frontier clusters, a distance field round every agent and the agents' territories - shared by the tests, and left unchanged."""
    if not _WORLD:
        from megastep_amd import cuda, modules
        from megastep_amd.demo import FloorCoverage
        torch.manual_seed(7); np.random.seed(7)
        env = FloorCoverage(8, n_agents=2, geometries=plans(8), shared=True, max_lifespan=10**6)
        env.reset()
        grid, maps = env.grid, env.maps
        territories = modules.Territories(env.core, grid)
        _WORLD.update(env=env, grid=grid, maps=maps, regions=cuda.regions(grid), clusters=maps.frontier_regions(),
                      around=cuda.distance_fields(grid, env.core.agents.positions), territories=territories,
                      seeds=cuda.basins(territories.near))
    return _WORLD


def test_on_eight_plans_the_regions_the_frontier_clusters_and_the_territories():
    from megastep_amd import cuda
    w = _world()
    grid, maps, around = w['grid'], w['maps'], w['around']
    # how much of each room has been seen, and how far each agent is from it
    rooms = w['regions'].zones(values=around, marks=maps, n_zones=32)
    assert rooms.ranked and rooms.n_fields == 2 and (rooms.n_labels, rooms.n_values, rooms.n_marks) == (1, 2, 1)
    got = _same(rooms)
    assert np.array_equal(got['n_zones'], _np(w['regions'].counts).repeat(2, 1)) and (got['marked'] <= got['cells']).all() and got['marked'].sum() > 1000
    assert np.isfinite(got['least']).any(-1).all()                        # (every agent stands in a room)
    # each agent's walk to the nearest cell of each frontier cluster, and which cell that is
    clusters = cuda.zones(w['clusters'], values=around, n_zones=64)
    got = _same(clusters)
    assert np.array_equal(got['n_zones'], _np(w['clusters'].counts).repeat(2, 1)) and (got['n_zones'] >= 1).all()
    reached = np.isfinite(got['least'])
    assert reached.any(-1).all() and np.array_equal(got['cells'][:, 0], got['cells'][:, 1])
    for n in range(8):                                                    # (the nearest cell is a cell of that cluster, at that distance)
        first, ny, nx = grid.cells(n)
        for a in range(2):
            cell, root = got['nearest'][n, a][reached[n, a]], got['roots'][n, a][reached[n, a]]
            assert np.array_equal(_np(w['clusters'].labels)[first + cell], root)
            assert np.array_equal(_np(around.values)[2*first + a*ny*nx + cell], got['least'][n, a][reached[n, a]])
    # within_marks: the nearest UNSEEN cell of each room (where=False)
    unseen = w['regions'].zones(values=around, marks=maps, n_zones=32, where=False, within_marks=True)
    got = _same(unseen)
    assert np.array_equal(got['marked'] + _np(rooms.marked), got['cells'])
    # the territories: direct by the agents' ids, ranked by the seeds' cells
    direct = w['territories'].basins.zones(values=cuda.cell_layer(maps.values.float()), n_zones=2)
    assert not direct.ranked
    got = _same(direct)
    assert np.array_equal(got['cells'], _np(w['territories'].basins.sizes)) and (got['roots'] == [0, 1]).all()
    ranked = w['seeds'].zones(values=w['territories'].near, n_zones=16)
    assert ranked.ranked
    got = _same(ranked)
    assert (got['least'][got['roots'] >= 0] == 0).all() and np.array_equal(got['nearest'][got['roots'] >= 0], got['roots'][got['roots'] >= 0])


def test_a_side_stream_and_a_captured_graph_replayed_after_new_marks():
    from megastep_amd import cuda
    w = _world()
    grid, around = w['grid'], w['around']
    maps = cuda.seen_maps(grid, 1, w['maps'].countable)
    maps.values.copy_(w['maps'].values)
    clusters = maps.frontier_regions()
    z = cuda.zones(clusters, values=around, marks=maps, n_zones=64)

    def chain():
        clusters.update(); z.update()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chain()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    first = _same(z)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                       # (two launches, one after the other: a linear graph)
        chain()
    rng = np.random.RandomState(8)
    seen = [first['cells']]
    for share in (.3, .6):
        maps.values[:grid.n_cells] |= _dev((rng.rand(grid.n_cells) < share).astype(np.uint8))
        graph.replay()
        torch.cuda.synchronize()
        got = {k: v.copy() for k, v in _result(z).items()}
        eager = cuda.zones(maps.frontier_regions(), values=around, marks=maps, n_zones=64)
        same(got, _result(eager))
        _same(z)
        assert not np.array_equal(got['cells'], seen[-1])
        seen.append(got['cells'])


def _several(costs):
    """(n_env,) bool: every agent of the env can walk to two zones or more."""
    return (torch.isfinite(costs).sum(-1) >= 2).all(-1)


def test_assignments_send_an_envs_agents_to_clusters_of_their_own():
    from megastep_amd import cuda, modules
    from megastep_amd.demo import FloorCoverage
    torch.manual_seed(5); np.random.seed(5)
    env = FloorCoverage(8, n_agents=2, geometries=plans(8), shared=True, max_lifespan=10**6)
    env.reset()
    grid, maps = env.grid, env.maps
    # choose on the device is the CPU loop's
    costs = choose_cases(3)
    choice, none = modules.Assignments.choose(_dev(costs))
    want = np.array([choose_by_loop(c) for c in costs])
    assert np.array_equal(_np(choice), want) and np.array_equal(_np(none), want < 0)
    everyone = torch.ones((8, 2), dtype=torch.bool, device='cuda')
    apart = 0
    for t in range(12):
        if t == 6:
            # env 0: nothing left to see; env 1: one cell - one cluster - left
            for n in (0, 1):
                first, ny, nx = grid.cells(n)
                maps.values[first:first + ny*nx] = 1
            first, ny, nx = grid.cells(1)
            cell = torch.nonzero(maps.countable[first:first + ny*nx])[ny*nx//40, 0]
            maps.values[first + cell] = 0
            env._assign(everyone)
            decision = env._assign_follower()                          # (the module is called once a step)
        else:
            decision = env.expert('assign')
        assign = env._assign
        if t == 0:
            assert decision.actions.shape == (8, 2) and decision.actions.dtype == torch.int64
            assert isinstance(assign, modules.Assignments) and isinstance(assign.zones, cuda.Zones) and assign.zones.least.shape == (8, 2, 64)
            assert assign.own.n_goals == 2 and assign.masks.n_fields == 2
        assert ((decision.actions >= 0) & (decision.actions < 7)).all()
        least = assign.zones.least
        _same(assign.zones)
        want = np.array([choose_by_loop(c) for c in _np(least)])
        assert np.array_equal(_np(assign.choice), want)
        several = _several(least)
        assert (assign.choice[several, 0] != assign.choice[several, 1]).all() and (assign.choice[several] >= 0).all()
        apart += int(several.sum())
        # the wanted labels are the chosen zones' roots, and an agent's mask is the cluster it was assigned, byte for byte
        roots = assign.zones.roots.gather(-1, assign.choice.clamp(min=0)[..., None])[..., 0]
        assert torch.equal(assign._wanted, torch.where(assign.choice < 0, -1, roots).int())
        for n in range(8):
            first, ny, nx = grid.cells(n)
            for a in range(2):
                mask = assign.masks.values[2*first + a*ny*nx:2*first + (a + 1)*ny*nx]
                labels = assign.clusters.labels[first:first + ny*nx]
                assert torch.equal(mask, ((labels == assign._wanted[n, a]) & (labels >= 0)).to(torch.uint8))
        own = assign.own.at(env.core.agents.positions)
        assert torch.equal(torch.isfinite(own), assign.choice >= 0)
        way, shared = assign.waypoints(), assign.fields.waypoints(env.core.agents.positions, goal=assign._field)
        lost = assign.choice < 0
        assert torch.equal(way[lost].view(torch.int32), shared[lost].view(torch.int32))
        if t == 6:
            assert assign.zones.n_zones[0].tolist() == [0, 0] and assign.choice[0].tolist() == [-1, -1] and torch.isnan(way[0]).all()
            assert assign.zones.n_zones[1].tolist() == [1, 1] and assign.zones.cells[1, :, 0].tolist() == [1, 1]
            can = torch.isfinite(least[1, :, 0])
            assert can.any() and (assign.choice[1][can] == 0).all() and (assign.choice[1][~can] == -1).all()      # (one cluster: whoever can walk there takes it)
        env.step(decision)
    print('envs, over 12 steps, whose two agents could each walk to two clusters or more - and were sent to different ones:', apart)
    assert apart >= 8
    with pytest.raises(RuntimeError, match='shared=True'):
        FloorCoverage(8, n_agents=2, geometries=plans(8)).expert('assign')


class _Expert:
    """An env whose step is the expert's: the decision handed in is ignored."""

    def __init__(self, env):
        self.env = env

    def __getattr__(self, name):
        return getattr(self.env, name)

    def step(self, decision):
        return self.env.step(self.env.expert('assign'))


def test_the_assign_expert_and_the_step_as_one_hip_graph_equal_the_eager_env():
    from megastep_amd import arrdict, graphs
    from megastep_amd.demo import FloorCoverage
    logs = []
    for graphed in (False, True):
        torch.manual_seed(3); np.random.seed(3)
        env = FloorCoverage(8, n_agents=2, geometries=plans(8), shared=True, max_lifespan=10**6, complete=.3)
        stepper = graphs.GraphedStep(_Expert(env), warmup=3) if graphed else _Expert(env)
        stepper.reset()
        nothing = arrdict.arrdict(actions=torch.zeros((8, 2), dtype=torch.long, device='cuda'))
        log = []
        # the graphed env's first step call is four steps: three of warm-up and the captured one
        for t in range(10 if graphed else 13):
            world = stepper.step(nothing)
            log.append((world.reward.clone(), world.reset.clone(), env.maps.values.clone(), env.core.agents.positions.clone(), env._assign.choice.clone()))
        logs.append(log)
    eager, graphed = logs
    for k in range(10):
        for got, want in zip(graphed[k], eager[k + 3]):
            assert torch.equal(got, want), k
    assert sum(float(log[0].sum()) for log in graphed) > 0
    assert not torch.equal(graphed[0][3], graphed[-1][3])                # (they moved)


def test_a_single_agent_is_assigned_its_nearest_cluster():
    from megastep_amd.demo import FloorCoverage
    torch.manual_seed(9); np.random.seed(9)
    env = FloorCoverage(8, n_agents=1, geometries=plans(8), shared=True, max_lifespan=10**6)
    env.reset()
    for t in range(5):
        decision = env.expert('assign')
        assert decision.actions.shape == (8, 1) and ((decision.actions >= 0) & (decision.actions < 7)).all()
        assign = env._assign
        least = assign.zones.least[:, 0]
        finite = torch.isfinite(least).any(-1)
        assert torch.equal(assign.choice[:, 0] >= 0, finite) and finite.any()
        picked = least.gather(-1, assign.choice.clamp(min=0))[:, 0]
        assert torch.equal(picked[finite], least.amin(-1)[finite])
        env.step(decision)
