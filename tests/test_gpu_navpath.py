"""Paths and look-ahead waypoints on the GPU: `DistanceFields.waypoints` and `.paths` equal AS BITS to the numpy statement of
the contract (tests/test_navpath_host.path_rule) on the fields the kernels themselves computed (which tests/test_gpu_navfield.py
holds to nav_rule, so no Dijkstra runs here); doors open and shut; `out=`, streams and graph capture; `modules.PathFollower`
and `PointGoal.expert`, eager and as one HIP graph, next to the compass policy of the PointGoal tests."""
import numpy as np
import pytest
import torch

from tests.test_navfield_host import CELL, RADIUS, F, _crossings, _two_rooms, bits, plans, spawn_points
from tests.test_navpath_host import path_rule
from tests.test_gpu_navfield import _custom, _draw_goals, _scenery, _walls

pytestmark = pytest.mark.gpu


def _worlds(grid, fields, e, cell=CELL):
    """path_rule's worlds of env e, one per field, and their hop tables - read back from the device."""
    geom = tuple(int(v) for v in grid.geom[e].cpu())
    free = grid.image(e).cpu().numpy()
    worlds = [(geom, cell, free, fields.image(e, g).cpu().numpy(), fields.goals[e, g].cpu().numpy()) for g in range(fields.n_goals)]
    return worlds, [path_rule.hops(w) for w in worlds]


def _rule(grid, fields, points, which, lookahead=None, max_points=None, cell=CELL):
    """What path_rule says for points (N, P, 2) following fields `which` (N, P): (waypoints, hops) or (paths, counts)."""
    n, p = points.shape[:2]
    G = fields.n_goals
    way, hops = np.full((n, p, 2), np.nan, F), np.full((n, p), -1, np.int32)
    paths, counts = np.full((n, p, max_points or 1, 2), np.nan, F), np.zeros((n, p), np.int32)
    for e in range(n):
        worlds, tables = _worlds(grid, fields, e, cell)
        for k in range(p):
            g = int(which[e, k])
            if not 0 <= g < G:
                continue
            if lookahead is not None:
                way[e, k], hops[e, k] = path_rule.waypoint(worlds[g], points[e, k], lookahead, tables[g])
            if max_points is not None:
                paths[e, k], counts[e, k] = path_rule.path(worlds[g], points[e, k], max_points, tables[g])
    return (way, hops) if max_points is None else (paths, counts)


def _equal(got, want):
    got = got.cpu().numpy()
    if got.dtype == np.float32:
        return np.array_equal(bits(got), bits(want))
    return np.array_equal(got, want)


def _points(sc, geoms, rng, spread=48, spawn=16):
    """(N, spread + spawn, 2): points over each plan's bounding box and 0.3 m beyond (some land in walls, some outside), then
    spawn-table points a few centimetres off their centres."""
    pts = np.empty((len(geoms), spread + spawn, 2), F)
    for e, g in enumerate(geoms):
        walls = _walls(sc, e)
        lo, hi = walls.reshape(-1, 2).min(0), walls.reshape(-1, 2).max(0)
        pts[e, :spread] = (lo - .3 + rng.uniform(0, 1, (spread, 2))*(hi - lo + .6)).astype(F)
        table = spawn_points(g)
        pts[e, spread:] = table[rng.choice(len(table), spawn)] + rng.uniform(-.05, .05, (spawn, 2)).astype(F)
    return pts


@pytest.mark.parametrize('oblique', [False, True])
def test_waypoints_and_paths_are_the_rules_bits(oblique):
    from megastep_amd import cuda
    geoms = plans(8, oblique)
    sc = _scenery(geoms)
    rng = np.random.RandomState(14 + oblique)
    grid = cuda.nav_grid(sc, clearance=RADIUS)
    fields = cuda.distance_fields(grid, torch.as_tensor(_draw_goals(geoms, 2, rng), device='cuda'))
    points = _points(sc, geoms, rng)
    which = rng.randint(0, 2, points.shape[:2]).astype(np.int32)
    pts, goal = torch.as_tensor(points, device='cuda'), torch.as_tensor(which, device='cuda')
    way, hops = fields.waypoints(pts, goal=goal, hops=True)
    found = fields.paths(pts, goal=goal, max_points=32)
    want_way, want_hops = _rule(grid, fields, points, which, lookahead=16)
    want_paths, want_counts = _rule(grid, fields, points, which, max_points=32)
    assert _equal(hops, want_hops) and _equal(way, want_way)
    assert _equal(found.counts, want_counts) and _equal(found.points, want_paths)
    # no path: exactly where the query says +inf
    assert torch.equal(hops < 0, torch.isinf(fields.at(pts, goal=goal))) and torch.equal(hops < 0, found.counts == 0)
    assert torch.equal(torch.isnan(way).any(-1), hops < 0)
    # the equality is not one of empty answers
    spawned = want_hops[:, 48:]
    assert (spawned >= 0).sum() >= .8*spawned.size, (spawned >= 0).sum()
    assert (spawned >= 2).sum() >= .5*(spawned >= 0).sum()
    assert (want_counts > 32).any() and (want_counts == 0).any()
    e, k = np.argwhere(want_counts > 0)[0]
    assert found.path(e, k).shape == (min(want_counts[e, k], 32), 2)


def test_a_large_plan_with_chains_of_hundreds_of_cells():
    from megastep_amd import cuda
    geoms = plans(1, large=True)
    sc = _scenery(geoms)
    rng = np.random.RandomState(18)
    grid = cuda.nav_grid(sc, clearance=RADIUS)
    fields = cuda.distance_fields(grid, torch.as_tensor(_draw_goals(geoms, 2, rng), device='cuda'))
    points = _points(sc, geoms, rng, spread=8, spawn=24)
    which = rng.randint(0, 2, points.shape[:2]).astype(np.int32)
    pts, goal = torch.as_tensor(points, device='cuda'), torch.as_tensor(which, device='cuda')
    found = fields.paths(pts, goal=goal, max_points=16)
    want_paths, want_counts = _rule(grid, fields, points, which, max_points=16)
    assert _equal(found.counts, want_counts) and _equal(found.points, want_paths)
    assert want_counts.max() > 100, want_counts.max()
    for L in (64, 1):
        way, hops = fields.waypoints(pts, goal=goal, lookahead=L, hops=True)
        want_way, want_hops = _rule(grid, fields, points, which, lookahead=L)
        assert _equal(hops, want_hops) and _equal(way, want_way), L
        assert want_hops.max() == 0 if L == 1 else want_hops.max() > 16  # (one candidate: x_0; 64: further than the default sees)


def test_through_the_door_when_it_is_open_and_nowhere_when_it_is_shut():
    from megastep_amd import cuda
    walls, a, b, (j0, j1) = _two_rooms()
    shut = np.concatenate([walls, np.array([[j0, j1]], F)])
    sc = _custom([walls, shut])
    grid = cuda.nav_grid(sc, clearance=RADIUS)
    fields = cuda.distance_fields(grid, torch.as_tensor(np.array([[b]]*2, F), device='cuda'))
    pts = torch.as_tensor(np.array([[a]]*2, F), device='cuda')
    way, hops = fields.waypoints(pts, hops=True)
    found = fields.paths(pts, max_points=256)
    # open: the path goes through the door, and neither it nor the way to the waypoint meets a wall
    path = found.path(0, 0).cpu().numpy()
    assert 2 < int(found.counts[0, 0]) == len(path) <= 256
    assert np.array_equal(path[0], a) and np.array_equal(path[-1], b)
    assert _crossings(path[:-1], path[1:], walls) == 0
    assert np.linalg.norm(path - (j0 + j1)/2, axis=1).min() <= .5
    assert int(hops[0, 0]) >= 2 and _crossings(a[None], way[0].cpu().numpy(), walls) == 0
    # shut: no path
    assert torch.isnan(way[1]).all() and int(hops[1, 0]) == -1 and int(found.counts[1, 0]) == 0
    assert torch.isnan(found.points[1]).all() and found.path(1, 0).shape == (0, 2)
    want_way, want_hops = _rule(grid, fields, pts.cpu().numpy(), np.zeros((2, 1), int), lookahead=16)
    assert _equal(way, want_way) and _equal(hops, want_hops)


def test_goal_indices_out_streams_and_a_second_agent():
    from megastep_amd import cuda
    geoms = plans(4)
    sc = _scenery(geoms, n_agents=2)
    rng = np.random.RandomState(19)
    grid = cuda.nav_grid(sc, clearance=RADIUS)
    fields = cuda.distance_fields(grid, torch.as_tensor(_draw_goals(geoms, 2, rng), device='cuda'))
    points = _points(sc, geoms, rng, spread=0, spawn=2)                  # two agents an env, each with a field of its own
    pts = torch.as_tensor(points, device='cuda')
    own = torch.tensor([[0, 1]]*4, device='cuda')
    way, hops = fields.waypoints(pts, hops=True)
    want_way, want_hops = _rule(grid, fields, points, own.cpu().numpy(), lookahead=16)
    assert _equal(way, want_way) and _equal(hops, want_hops) and (want_hops >= 0).sum() >= 6
    named, named_hops = fields.waypoints(pts, goal=own, hops=True)
    assert torch.equal(named.view(torch.int32), way.view(torch.int32)) and torch.equal(named_hops, hops)
    swapped = fields.waypoints(pts, goal=1 - own)
    assert _equal(swapped, _rule(grid, fields, points, 1 - own.cpu().numpy(), lookahead=16)[0])
    assert not torch.equal(swapped.view(torch.int32), way.view(torch.int32))
    # no such field
    seven = torch.full((4, 2), 7, dtype=torch.int64, device='cuda')
    none, none_hops = fields.waypoints(pts, goal=seven, hops=True)
    assert torch.isnan(none).all() and (none_hops == -1).all() and (fields.paths(pts, goal=seven, max_points=4).counts == 0).all()
    assert torch.isnan(fields.paths(pts, goal=seven, max_points=4).points).all()
    # out=, and a side stream
    out = torch.zeros_like(way)
    assert fields.waypoints(pts, out=out) is out and torch.equal(out.view(torch.int32), way.view(torch.int32))
    with pytest.raises(RuntimeError, match='out'):
        fields.waypoints(pts, out=torch.zeros(4, 2, device='cuda'))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        there, there_hops = fields.waypoints(pts, hops=True)
        paths = fields.paths(pts, max_points=8)
    side.synchronize()
    assert torch.equal(there.view(torch.int32), way.view(torch.int32)) and torch.equal(there_hops, hops)
    assert _equal(paths.counts, _rule(grid, fields, points, own.cpu().numpy(), max_points=8)[1])


def test_a_captured_call_follows_points_and_fields_changed_in_place():
    from megastep_amd import cuda
    geoms = plans(4)
    sc = _scenery(geoms)
    rng = np.random.RandomState(23)
    grid = cuda.nav_grid(sc, clearance=RADIUS)
    goals = torch.as_tensor(_draw_goals(geoms, 2, rng), device='cuda')
    fields = cuda.distance_fields(grid, goals)
    pts = torch.as_tensor(_points(sc, geoms, rng, spread=0, spawn=2), device='cuda')
    mask = torch.zeros((4, 2), dtype=torch.bool, device='cuda')
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fields.update(goals, mask); fields.waypoints(pts, hops=True)
    torch.cuda.current_stream().wait_stream(side)
    with torch.cuda.graph(graph):
        fields.update(goals, mask)
        way, hops = fields.waypoints(pts, hops=True)
    different = 0
    last = None
    for trial in range(3):
        goals.copy_(torch.as_tensor(_draw_goals(geoms, 2, rng), device='cuda'))
        pts.copy_(torch.as_tensor(_points(sc, geoms, rng, spread=0, spawn=2), device='cuda'))
        mask.copy_(torch.as_tensor(rng.rand(4, 2) < .6, device='cuda'))
        graph.replay()
        got, got_hops = way.clone(), hops.clone()
        fields.update(goals, mask)                                      # (the same again, eagerly: an update is idempotent)
        want, want_hops = fields.waypoints(pts, hops=True)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and torch.equal(got_hops, want_hops)
        assert _equal(got, _rule(grid, fields, pts.cpu().numpy(), np.array([[0, 1]]*4), lookahead=16)[0])
        different += last is not None and not torch.equal(last, got.view(torch.int32))
        last = got.view(torch.int32).clone()
    assert different == 2 and (got_hops >= 0).any()


def _rollout(env, steps, policy, seed=1):
    """`steps` steps of `env` under `policy` ('expert': env.expert(), nothing random; 'compass': the PointGoal tests' policy, one
    step in four random). The log holds what those tests' holds, and where the agents stood."""
    from megastep_amd import arrdict
    rng = np.random.RandomState(seed)
    n, a = env.core.n_envs, env.core.n_agents
    world = env.reset()
    frame = lambda world: arrdict.arrdict(reset=world.reset.clone(), reward=world.reward.clone(), g=env._distance.clone(),
                                          stranded=env._goals.stranded.clone(), goal=world.obs.goal.clone(),
                                          at=env.core.agents.positions.clone())
    log = [frame(world)]
    for t in range(steps):
        if policy == 'expert':
            decision = env.expert()
        else:
            x, y = (world.obs.goal[..., k].cpu().numpy() for k in (0, 1))
            seek = np.where((y > 0) & (np.abs(x) < y), 1, np.where(x < 0, 5, 6))
            actions = np.where(rng.rand(n, a) < .25, rng.randint(0, 7, (n, a)), seek)
            decision = arrdict.arrdict(actions=torch.as_tensor(actions, device='cuda'))
        world = env.step(decision)
        log.append(frame(world))
    return log


def _score(env, log, check=False):
    """(episodes, arrivals, mean walked / walking distance at the start, mean walked / walking distance covered) over the
    episodes of the log in which nobody was stranded; the ratios over those that arrived.  check: the env's promises."""
    reset = torch.stack([w.reset for w in log]).cpu().numpy()
    reward = torch.stack([w.reward for w in log])[..., 0].cpu().numpy().astype(np.float64)
    g = torch.stack([w.g for w in log])[..., 0].cpu().numpy().astype(np.float64)
    stranded = torch.stack([w.stranded for w in log])[..., 0].cpu().numpy()
    at = torch.stack([w.at for w in log])[:, :, 0].cpu().numpy().astype(np.float64)
    episodes = arrivals = 0
    of_start, of_covered = [], []
    for e in range(reset.shape[1]):
        starts = list(np.nonzero(reset[:, e])[0]) + [len(log)]
        for s, t in zip(starts[:-1], starts[1:]):
            if stranded[s:t, e].any():
                continue
            episodes += 1
            if check:
                assert reward[s, e] == 0
                assert abs(reward[s:t, e].sum() - (g[s, e] - g[t - 1, e])) <= 200*2.**-20
                assert (g[s:t - 1, e] >= env.arrive).all()
            if g[t - 1, e] < env.arrive:
                arrivals += 1
                walked = np.linalg.norm(np.diff(at[s:t, e], axis=0), axis=1).sum()
                of_start.append(walked/g[s, e]); of_covered.append(walked/(g[s, e] - g[t - 1, e]))
        if check:
            for t in range(1, len(log)):
                if g[t - 1, e] < env.arrive and not stranded[t - 1, e]:
                    assert reset[t, e]
    if check:
        assert reset[0].all() and np.isfinite(reward).all() and (np.isfinite(g) | stranded).all()
    return episodes, arrivals, float(np.mean(of_start)) if of_start else float('nan'), float(np.mean(of_covered)) if of_covered else float('nan')


def test_the_expert_arrives_at_least_as_often_as_the_compass_policy():
    """PointGoal(64), 200 steps, once under env.expert() and once under the compass policy of the PointGoal tests: the expert's
    arrivals are at least the compass's; rewards still telescope and whoever arrives starts over."""
    from megastep_amd.demo import PointGoal
    results = {}
    for policy in ('expert', 'compass'):
        torch.manual_seed(3); np.random.seed(3)
        env = PointGoal(64, geometries=plans(64), bonus=0., max_lifespan=120)
        log = _rollout(env, 200, policy)
        results[policy] = _score(env, log, check=True)
        episodes, arrivals, of_start, of_covered = results[policy]
        print(f'PointGoal(64), 200 steps, {policy}: {episodes} episodes, {arrivals} arrivals, walked/start distance {of_start:.3f}, '
              f'walked/distance covered {of_covered:.3f}')
        if policy == 'expert':
            actions = env.expert().actions
            assert actions.shape == (64, 1) and actions.dtype == torch.int64 and ((actions >= 0) & (actions < 7)).all()
    assert results['expert'][0] > 64 and results['expert'][1] >= results['compass'][1], results


class _Expert:
    """An env whose step is the expert's: the decision handed in is ignored."""

    def __init__(self, env):
        self.env = env

    def __getattr__(self, name):
        return getattr(self.env, name)

    def step(self, decision):
        return self.env.step(self.env.expert())


def test_the_expert_and_the_step_as_one_hip_graph_equal_the_eager_env():
    from megastep_amd import arrdict, graphs
    from megastep_amd.demo import PointGoal
    logs = []
    for graphed in (False, True):
        torch.manual_seed(3); np.random.seed(3)
        env = PointGoal(64, geometries=plans(64), max_lifespan=10**6)
        stepper = graphs.GraphedStep(_Expert(env), warmup=3) if graphed else _Expert(env)
        world = stepper.reset()
        nothing = arrdict.arrdict(actions=torch.zeros((64, 1), dtype=torch.long, device='cuda'))
        log = []
        for t in range(60 if graphed else 63):
            world = stepper.step(nothing)
            log.append(arrdict.arrdict(reset=world.reset.clone(), reward=world.reward.clone(), g=env._distance.clone(),
                                       goal=world.obs.goal.clone(), at=env.core.agents.positions.clone()))
        logs.append(log)
    eager, graphed = logs
    # the graphed env's first step call is four steps (three of warm-up and the captured one): its k-th is the eager env's k + 3
    for k in range(len(graphed)):
        for name in ('reset', 'reward', 'g', 'goal', 'at'):
            assert torch.equal(graphed[k][name], eager[k + 3][name]), (k, name)
    assert any(w.reset.any() for w in graphed[1:])                       # somebody arrived and started over inside the graph
