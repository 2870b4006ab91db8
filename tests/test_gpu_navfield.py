"""Shortest-path distance fields on the GPU: `cuda.nav_grid`, `cuda.distance_fields`, `DistanceFields.at` equal AS BITS to the
numpy statement of the contract (tests/test_navfield_host.nav_rule: free cells, a heap Dijkstra with binary32 additions, the
anchors' query) - the relaxation's result does not depend on its schedule, so the kernel is held to equality, not to a
tolerance; masks, `out=`, streams and graph capture; `modules.Goals`; and the `PointGoal` env, eager and as one HIP graph."""
import numpy as np
import pytest
import torch

from tests.test_navfield_host import CELL, RADIUS, F, bits, nav_rule, plans, spawn_points, _two_rooms

pytestmark = pytest.mark.gpu


def _scenery(geoms, n_agents=1):
    from megastep_amd import scene
    return scene.scenery(geoms, n_agents, device='cuda', random=np.random.RandomState(0), bake=False)


def _walls(sc, e):
    return sc.lines[e][sc.n_agents*sc.model.shape[0]:].cpu().numpy()


def _draw_goals(geoms, n_goals, rng):
    """(N, G, 2) float32: spawn-table points, a few centimetres off their cell centres."""
    goals = np.empty((len(geoms), n_goals, 2), F)
    for e, g in enumerate(geoms):
        pts = spawn_points(g)
        goals[e] = pts[rng.choice(len(pts), n_goals)] + rng.uniform(-.09, .09, (n_goals, 2)).astype(F)
    return goals


def _check(sc, grid, fields, goals, rng, n_points=48, worth=None, cell=CELL, clearance=RADIUS):
    """Free cells, every field and a batch of queries of every env against nav_rule, as bits. Returns how many goals had an
    anchor and a finite region of more than 500 cells."""
    n, G = goals.shape[:2]
    geom = grid.geom.cpu().numpy()
    points = np.empty((n, n_points, 2), F)
    which = rng.randint(0, G, (n, n_points)).astype(np.int32)
    for e in range(n):
        walls = _walls(sc, e)
        lo, hi = walls.reshape(-1, 2).min(0), walls.reshape(-1, 2).max(0)
        points[e] = (lo - .3 + rng.uniform(0, 1, (n_points, 2))*(hi - lo + .6)).astype(F)
    got_q = fields.at(torch.as_tensor(points, device='cuda'), goal=torch.as_tensor(which, device='cuda')).cpu().numpy()
    good = 0
    for e in range(n):
        walls = _walls(sc, e)
        ge = tuple(int(v) for v in geom[e])
        assert ge == nav_rule.geometry(walls, cell)
        free = nav_rule.free(walls, ge, cell, clearance)
        assert np.array_equal(grid.image(e).cpu().numpy(), free), e
        graph = nav_rule._neighbours(free, cell)
        want = [nav_rule.field(free, ge, cell, goals[e, g], graph) for g in range(G)]
        for g in range(G):
            got = fields.image(e, g).cpu().numpy()
            assert np.array_equal(bits(got), bits(want[g])), (e, g, int((bits(got) != bits(want[g])).sum()))
            good += bool(nav_rule.anchors(goals[e, g], ge, cell, free)) and int(np.isfinite(want[g]).sum()) > 500
        want_q = np.array([nav_rule.query(want[which[e, k]], ge, cell, free, points[e, k]) for k in range(n_points)], F)
        assert np.array_equal(bits(got_q[e]), bits(want_q)), e
    return good


def test_the_box():
    from megastep_amd import cuda, toys
    sc = _scenery([toys.box()])
    grid = cuda.nav_grid(sc, clearance=RADIUS)
    x, y = nav_rule.centres(tuple(int(v) for v in grid.geom[0].cpu()), CELL)
    goals = np.array([[[x[len(x)//2], y[len(y)//2]], [2.313, 4.071]]], F)
    fields = cuda.distance_fields(grid, torch.as_tensor(goals, device='cuda'), passes=True)
    assert _check(sc, grid, fields, goals, np.random.RandomState(0)) == 2
    assert fields.image(0, 0).min() == 0 and (fields.passes > 10).all()
    a = torch.tensor([[[1.5, 1.5]]], device='cuda')
    b = torch.tensor([[[4.5, 3.5]]], device='cuda')
    d = float(cuda.geodesic(grid, a, b))
    assert 13**.5 <= d <= 1.09*13**.5                                     # open space: the octile metric, within 8 % of the line


@pytest.mark.parametrize('oblique', [False, True])
def test_fields_and_queries_are_the_rules_bits(oblique):
    """8 plans x 2 goals from the spawn table: at least 90 % of the goals have an anchor and a region of more than 500 cells, so
    the equality is not one of empty fields."""
    from megastep_amd import cuda
    geoms = plans(8, oblique)
    sc = _scenery(geoms)
    rng = np.random.RandomState(4 + oblique)
    goals = _draw_goals(geoms, 2, rng)
    grid = cuda.nav_grid(sc, clearance=RADIUS)
    fields = cuda.distance_fields(grid, torch.as_tensor(goals, device='cuda'))
    assert _check(sc, grid, fields, goals, rng) >= .9*16


def test_envs_that_share_a_floorplan_and_a_second_agent():
    from megastep_amd import cuda, cubicasa
    geoms = cubicasa.sample(6, seed=7, n_unique=4)                       # three plans, each twice
    sc = _scenery(geoms, n_agents=2)
    assert sc.geom is not None and len(set(sc.geom.tolist())) < 6
    rng = np.random.RandomState(6)
    goals = _draw_goals(geoms, 3, rng)
    grid = cuda.nav_grid(sc, clearance=RADIUS)
    fields = cuda.distance_fields(grid, torch.as_tensor(goals, device='cuda'))
    assert _check(sc, grid, fields, goals, rng) >= 14


def test_a_large_plan_relaxes_in_global_memory_to_the_same_bits():
    from megastep_amd import cuda
    geoms = plans(1, large=True)
    sc = _scenery(geoms)
    grid = cuda.nav_grid(sc, clearance=RADIUS)
    assert grid.n_cells > 40000                                          # beyond what 160 KiB of LDS hold
    rng = np.random.RandomState(8)
    goals = _draw_goals(geoms, 2, rng)
    fields = cuda.distance_fields(grid, torch.as_tensor(goals, device='cuda'))
    assert _check(sc, grid, fields, goals, rng) >= 1


def _custom(walls_per_env):
    from megastep_amd import arrdict
    geoms = [arrdict.arrdict(walls=np.asarray(w, float), lights=np.array([[2., 2.]]), masks=np.ones((4, 4), np.int16), res=.2)
             for w in walls_per_env]
    return _scenery(geoms)


def test_goals_without_an_anchor_and_goals_in_a_closed_room():
    from megastep_amd import cuda
    walls, a, b, (j0, j1) = _two_rooms()
    shut = np.concatenate([walls, np.array([[j0, j1]], F)])
    sc = _custom([walls, shut])
    grid = cuda.nav_grid(sc, clearance=RADIUS)
    # env 0 (door open) and env 1 (door shut): a goal in the right room, one far outside, one that is not a number, one in a wall
    goals = np.array([[b, [50., 50.], [np.nan, 2.], [1., 3.]]]*2, F)
    fields = cuda.distance_fields(grid, torch.as_tensor(goals, device='cuda'))
    _check(sc, grid, fields, goals, np.random.RandomState(1))
    for e in range(2):
        for g in (1, 2, 3):
            assert torch.isinf(fields.image(e, g)).all()
    pts = torch.as_tensor(np.array([[a, b]]*2, F), device='cuda')
    d = fields.at(pts, goal=torch.zeros((2, 2), dtype=torch.int64, device='cuda')).cpu().numpy()
    assert np.isfinite(d[0]).all() and d[0, 0] > np.linalg.norm(a - b) + .5          # through the door, not through the wall
    assert np.isinf(d[1, 0]) and np.isfinite(d[1, 1])                                # shut: finite in the room, +inf outside
    inside = torch.isfinite(fields.image(1, 0))
    assert 500 < int(inside.sum()) < int(torch.isfinite(fields.image(0, 0)).sum())
    assert torch.isinf(fields.at(pts, goal=torch.full((2, 2), 7, dtype=torch.int64, device='cuda'))).all()      # no such field


def test_mask_out_and_streams():
    from megastep_amd import cuda
    geoms = plans(4)
    sc = _scenery(geoms)
    rng = np.random.RandomState(9)
    first, second = _draw_goals(geoms, 2, rng), _draw_goals(geoms, 2, rng)
    grid = cuda.nav_grid(sc, clearance=RADIUS)
    fields = cuda.distance_fields(grid, torch.as_tensor(first, device='cuda'))
    reference = cuda.distance_fields(grid, torch.as_tensor(second, device='cuda'))
    sentinel = -7.25
    fields.values.fill_(sentinel)
    mask = torch.tensor([[True, False], [False, False], [False, True], [True, True]], device='cuda')
    same = cuda.distance_fields(grid, torch.as_tensor(second, device='cuda'), mask=mask, out=fields)
    assert same is fields
    for e in range(4):
        for g in range(2):
            if mask[e, g]:
                assert torch.equal(fields.image(e, g).view(torch.int32), reference.image(e, g).view(torch.int32))
                assert torch.equal(fields.goals[e, g].cpu(), torch.as_tensor(second[e, g]))
            else:
                assert (fields.image(e, g) == sentinel).all()
                assert torch.equal(fields.goals[e, g].cpu(), torch.as_tensor(first[e, g]))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = cuda.distance_fields(grid, torch.as_tensor(second, device='cuda'))
        pts = torch.as_tensor(first, device='cuda')
        q = other.at(pts)
    side.synchronize()
    assert torch.equal(other.values.view(torch.int32), reference.values.view(torch.int32))
    assert torch.equal(q.view(torch.int32), reference.at(pts).view(torch.int32))
    out = torch.empty_like(q)
    assert reference.at(pts, out=out) is out and torch.equal(out, q)


def _goals_world(n=8, n_agents=2):
    from megastep_amd import core, cuda, modules
    from tests import util
    geoms = plans(n)
    sc = _scenery(geoms, n_agents)
    c = core.Core(sc, res=64)
    util.spawn(c, geoms, seed=3)
    grid = cuda.nav_grid(sc, clearance=RADIUS)
    np.random.seed(5)
    return geoms, c, modules.Goals(geoms, c, grid, candidates=8, min_distance=1.)


def test_goals_are_reachable_and_a_captured_draw_equals_an_eager_one():
    from tests import util
    geoms, c, goals = _goals_world()
    everyone = c.agent_full(True)
    goals(everyone)
    d = goals.distances()
    assert (torch.isfinite(d) | goals.stranded).all() and (d[~goals.stranded] >= 1.).all()
    assert goals.stranded.float().mean() < .2
    obs = goals.observation()
    assert obs.shape == (8, 2, 3) and torch.isfinite(obs).all()
    # the promise, against the rule: the distance the module reports is nav_rule's from the agent to its goal
    e = 3
    ge = tuple(int(v) for v in goals.grid.geom[e].cpu())
    free = nav_rule.free(_walls(c.scenery, e), ge, CELL, RADIUS)
    want = nav_rule.query(nav_rule.field(free, ge, CELL, goals.goals[e, 1].cpu().numpy()), ge, CELL, free, c.agents.positions[e, 1].cpu().numpy())
    assert bits(d[e, 1].cpu().numpy()) == bits(want)

    # captured: a draw for some agents and the distances; goals and positions change between replays
    mask = c.agent_full(False)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        goals(mask); goals.distances()
    torch.cuda.current_stream().wait_stream(side)
    with torch.cuda.graph(graph):
        goals(mask)
        captured = goals.distances()
    rng = np.random.RandomState(2)
    for trial in range(3):
        mask.copy_(torch.as_tensor(rng.rand(8, 2) < .5, device='cuda'))
        util.spawn(c, geoms, seed=10 + trial)
        draws, held, stranded = goals._draws.clone(), goals.goals.clone(), goals.stranded.clone()
        graph.replay()
        got, got_goals, got_stranded = captured.clone(), goals.goals.clone(), goals.stranded.clone()
        goals._draws.copy_(draws); goals.goals.copy_(held); goals.stranded.copy_(stranded)       # the same draw again, eagerly
        goals(mask)
        want = goals.distances()
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
        assert torch.equal(got_goals, goals.goals) and torch.equal(got_stranded, goals.stranded)
        assert torch.equal(goals.goals[~mask], held[~mask])
        assert (goals.goals[mask & ~goals.stranded] != held[mask & ~goals.stranded]).any()


def _rollout(env, steps, seed, lead=0, compass=True):
    from megastep_amd import arrdict
    rng = np.random.RandomState(seed)
    n, a = env.core.n_envs, env.core.n_agents
    world = env.reset()
    log = [arrdict.arrdict(reset=world.reset.clone(), reward=world.reward.clone(), g=env._distance.clone(),
                           stranded=env._goals.stranded.clone(), goal=world.obs.goal.clone())]
    for t in range(steps):
        # a compass policy, so that agents get somewhere: turn until the goal is ahead, then walk (modules.to_local_frame: x to the
        # right, y ahead); one step in four is random.  The first `lead` steps forward for all (a graphed env warms up under its
        # first actions).
        x, y = (world.obs.goal[..., k].cpu().numpy() for k in (0, 1))
        seek = np.where((y > 0) & (np.abs(x) < y), 1, np.where(x < 0, 5, 6))
        actions = np.where(rng.rand(n, a) < (.25 if compass else 1.), rng.randint(0, 7, (n, a)), seek) if t >= lead else np.ones((n, a), int)
        world = env.step(arrdict.arrdict(actions=torch.as_tensor(actions, device='cuda')))
        log.append(arrdict.arrdict(reset=world.reset.clone(), reward=world.reward.clone(), g=env._distance.clone(),
                                   stranded=env._goals.stranded.clone(), goal=world.obs.goal.clone()))
    return log


@pytest.mark.parametrize('compass', [False, True])
def test_pointgoal_rewards_telescope_and_every_agent_has_somewhere_to_go(compass):
    """200 steps of PointGoal(64) under random actions, and under a policy that walks towards the goal (so that agents arrive)."""
    from megastep_amd.demo import PointGoal
    torch.manual_seed(3); np.random.seed(3)
    env = PointGoal(64, geometries=plans(64), bonus=0., max_lifespan=120)
    assert env.obs_space.goal.shape == (1, 3) and env.obs_space.rgb.shape == (1, 3, 1, 64)
    log = _rollout(env, 200, seed=1, compass=compass)
    reset = torch.stack([w.reset for w in log]).cpu().numpy()           # (T, N)
    reward = torch.stack([w.reward for w in log])[..., 0].cpu().numpy().astype(np.float64)
    g = torch.stack([w.g for w in log])[..., 0].cpu().numpy().astype(np.float64)
    stranded = torch.stack([w.stranded for w in log])[..., 0].cpu().numpy()
    assert reset[0].all() and np.isfinite(reward).all()
    assert (np.isfinite(g) | stranded).all()                             # the goal rule's promise
    assert stranded.mean() < .05
    arrivals = episodes = 0
    for e in range(64):
        starts = list(np.nonzero(reset[:, e])[0]) + [len(log)]
        for s, t in zip(starts[:-1], starts[1:]):
            if stranded[s:t, e].any():
                continue
            episodes += 1
            assert reward[s, e] == 0
            assert abs(reward[s:t, e].sum() - (g[s, e] - g[t - 1, e])) <= 200*2.**-20
            assert (g[s:t - 1, e] >= env.arrive).all()                   # an episode goes on only while the goal is not reached ...
            arrivals += g[t - 1, e] < env.arrive
        for t in range(1, len(log)):                                     # ... and whoever arrived starts over at the next step
            if g[t - 1, e] < env.arrive and not stranded[t - 1, e]:
                assert reset[t, e]
    assert episodes > 64 and (arrivals > 0 or not compass)
    print(f'PointGoal(64), compass={compass}: {episodes} episodes, {arrivals} arrivals, stranded share {stranded.mean():.4f}')
    state = env.state(0)
    assert state.goals.goals.shape == (1, 2) and state.distance.shape == (1,)


def test_pointgoal_as_a_hip_graph_equals_the_eager_env():
    """Nothing in a PointGoal step but the lifespans draws random numbers; with lifespans out of reach the graphed rollout is the
    eager one, bit for bit."""
    from megastep_amd import graphs
    from megastep_amd.demo import PointGoal
    logs = []
    for graphed in (False, True):
        torch.manual_seed(3); np.random.seed(3)
        env = PointGoal(64, geometries=plans(64), max_lifespan=10**6)
        logs.append(_rollout(graphs.GraphedStep(env, warmup=3), 200, seed=1, lead=4) if graphed else _rollout(env, 203, seed=1, lead=7))
    eager, graphed = logs
    # the graphed env's first step call is four steps (three of warm-up and the captured one) under the rollout's first actions:
    # its k-th call is the eager env's step k + 3
    for k in range(1, len(graphed) - 3):
        for name in ('reset', 'reward', 'g', 'stranded', 'goal'):
            assert torch.equal(graphed[k][name], eager[k + 3][name]), (k, name)
    print('graphed PointGoal(64): resets after the first step:', sum(int(w.reset.sum()) for w in graphed[2:]))
    assert any(w.reset.any() for w in graphed[2:])
