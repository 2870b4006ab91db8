"""Seeded fields on the GPU: `cuda.seeded_fields` and `SeenMaps.frontier_fields` equal AS BITS to the numpy statement of the
contract (tests/test_navseed_host.seed_rule) - fields, seed counts and queries - with the seeds of real seen maps; the
global-memory path of a large plan; `waypoints` and `paths` on them; that seeing more never brings the frontier nearer; `mask`,
`out=`, streams and graph capture; and `FloorCoverage.expert`, next to a random policy and as one HIP graph."""
import numpy as np
import pytest
import torch

from tests.test_navfield_host import CELL, RADIUS, F, bits, nav_rule, plans
from tests.test_navseed_host import seed_rule
from tests.test_gpu_navseen import _core, _np
from tests.test_gpu_navpath import _points

pytestmark = pytest.mark.gpu


def _env(grid, e):
    """(geom, free (ny, nx) bool, slice of the env's cells in the grid's flat layout) - read back from the device."""
    first, ny, nx = grid.cells(e)
    return tuple(int(v) for v in grid.geom[e].cpu()), _np(grid.image(e)), slice(first, first + ny*nx)


def _rule_fields(grid, marks, n_fields, where, among, cell=CELL):
    """seed_rule's fields for marks in the fields' layout: ([env][field] (ny, nx) float32, (N, G) seed counts)."""
    marks, among = _np(marks), None if among is None else _np(among)
    fields, counts = [], np.zeros((grid.n_envs, n_fields), np.int32)
    for e in range(grid.n_envs):
        geom, free, cells = _env(grid, e)
        graph = nav_rule._neighbours(free, cell) if free.size else None
        row = []
        for g in range(n_fields):
            at = n_fields*cells.start + g*free.size
            seeds = seed_rule.seeds(free, marks[at:at + free.size].reshape(free.shape), where, None if among is None else among[cells].reshape(free.shape))
            counts[e, g] = seeds.sum()
            row.append(seed_rule.field(free, cell, seeds, graph))
        fields.append(row)
    return fields, counts


def _fields_equal(grid, got, want):
    """Are the device's fields the rule's, as bits; returns how many are worth the comparison (finite on more than 500 cells)."""
    worth = 0
    for e in range(grid.n_envs):
        for g in range(got.n_goals):
            have = _np(got.image(e, g))
            assert np.array_equal(bits(have), bits(want[e][g])), (e, g, int((bits(have) != bits(want[e][g])).sum()))
            worth += np.isfinite(want[e][g]).sum() > 500
    return worth


def _queries_equal(grid, got, want, points, which, cell=CELL):
    """`at` for points (N, P, 2) against fields `which` (N, P), out-of-range indices included, as bits."""
    have = got.at(torch.as_tensor(points, device='cuda'), goal=torch.as_tensor(which, device='cuda'))
    rule = np.full(which.shape, np.inf, F)
    for e in range(grid.n_envs):
        geom, free, _ = _env(grid, e)
        for k in range(which.shape[1]):
            if 0 <= which[e, k] < got.n_goals:
                rule[e, k] = seed_rule.query((geom, cell, free, want[e][which[e, k]]), points[e, k])
    assert np.array_equal(bits(_np(have)), bits(rule))
    return rule


_NINE = {}


def _nine():
    """toys.box() and eight plans (four plain, four oblique), two agents each with a seen map of its own, the floor that counts
    what can be walked to from the first agent, one frame marked - and the second frame's agents, for later."""
    if not _NINE:
        from megastep_amd import cuda, toys
        from megastep_amd.demo.envs.floorcoverage import reachable
        geoms = [toys.box()] + plans(4) + plans(4, oblique=True)
        c = _core(geoms, 2, 64)
        grid = cuda.nav_grid(c.scenery, clearance=RADIUS)
        countable = reachable(grid, c.agents.positions[:, 0])
        maps = cuda.seen_maps(grid, 2, countable)
        maps.mark_render(c.agents, cuda.render(c.scenery, c.agents, fields=('distances',)), max_range=4.)
        _NINE.update(core=c, geoms=geoms, grid=grid, maps=maps, first=maps.values.clone())
    return _NINE


def _second_frame(w, maps=None, cover=None):
    """The agents turned by 100 degrees: what they see then is marked on `maps`, or by the Coverage module `cover`."""
    from megastep_amd import cuda, modules
    c = w['core']
    angles = c.agents.angles.clone()
    c.agents.angles[:] = angles + 100.
    if cover is not None:
        cover(modules.render(c, fields=('distances',)))
    else:
        maps.mark_render(c.agents, cuda.render(c.scenery, c.agents, fields=('distances',)), max_range=4.)
    c.agents.angles[:] = angles


def _first_maps(w):
    """A fresh SeenMaps holding the first frame's marks."""
    from megastep_amd import cuda
    maps = cuda.seen_maps(w['grid'], 2, w['maps'].countable)
    maps.values.copy_(w['first'])
    return maps


@pytest.mark.parametrize('where', [False, True])
def test_seeded_fields_are_the_rules_bits_on_real_seen_maps(where):
    """where=False: the frontier - the countable cells a map has not seen - through frontier_fields; where=True: the seen
    cells themselves, through seeded_fields."""
    from megastep_amd import cuda
    w = _nine()
    grid, maps = w['grid'], _first_maps(w)
    if where:
        got = cuda.seeded_fields(grid, maps.values, 2, where=True, passes=True)
        want, counts = _rule_fields(grid, maps.values, 2, 1, None)
    else:
        got = maps.frontier_fields(passes=True)
        want, counts = _rule_fields(grid, maps.values, 2, 0, maps.countable)
    assert got.n_seeds.dtype == torch.int32 and np.array_equal(_np(got.n_seeds), counts), (_np(got.n_seeds), counts)
    worth = _fields_equal(grid, got, want)
    good = sum(counts[e, g] > 0 and np.isfinite(want[e][g]).sum() > 500 for e in range(9) for g in range(2))
    print(f'where={where}: {good} of 18 fields have a seed and more than 500 finite cells; seeds {counts.reshape(-1).tolist()}, '
          f'passes {_np(got.passes).reshape(-1).tolist()}')
    assert good >= .9*18 and worth >= good
    assert (_np(got.passes) >= 2).all()
    rng = np.random.RandomState(3 + where)
    points = _points(w['core'].scenery, w['geoms'], rng, spread=16, spawn=16)
    which = rng.randint(0, 2, points.shape[:2]).astype(np.int32)
    which[:, ::9] = [[-1, 2, 7, -2**31]]
    rule = _queries_equal(grid, got, want, points, which)
    assert np.isfinite(rule).sum() > .3*rule.size and np.isinf(rule[:, ::9]).all() and (rule == 0).sum() < np.isfinite(rule).sum()


def test_a_large_plan_relaxes_in_global_memory_to_the_same_bits():
    from megastep_amd import cuda
    geoms = plans(1, large=True)
    c = _core(geoms, 2, 256, seed=3)
    grid = cuda.nav_grid(c.scenery, clearance=RADIUS)
    assert grid.n_cells > 40000 and grid._max_framed > (160*1024 - 64)//5          # (more than the largest LDS holds)
    maps = cuda.seen_maps(grid, 2)
    maps.mark_render(c.agents, cuda.render(c.scenery, c.agents, fields=('distances',)))
    frontier = maps.frontier_fields(passes=True)
    want, counts = _rule_fields(grid, maps.values, 2, 0, maps.countable)
    assert np.array_equal(_np(frontier.n_seeds), counts) and (counts > 1000).all()
    assert _fields_equal(grid, frontier, want) == 2
    seen = cuda.seeded_fields(grid, maps.values, 2, where=True)
    want, counts = _rule_fields(grid, maps.values, 2, 1, None)
    assert np.array_equal(_np(seen.n_seeds), counts) and (counts > 100).all()
    assert _fields_equal(grid, seen, want) == 2


def _follow_rule(grid, fields, points, which, lookahead=None, max_points=None, cell=CELL):
    """What seed_rule says for points (N, P, 2) following fields `which` (N, P) of the device's own fields."""
    n, p = points.shape[:2]
    way, hops = np.full((n, p, 2), np.nan, F), np.full((n, p), -1, np.int32)
    paths, counts = np.full((n, p, max_points or 1, 2), np.nan, F), np.zeros((n, p), np.int32)
    for e in range(n):
        geom, free, _ = _env(grid, e)
        worlds = [(geom, cell, free, _np(fields.image(e, g))) for g in range(fields.n_goals)]
        tables = [seed_rule.hops(world) for world in worlds]
        for k in range(p):
            g = int(which[e, k])
            if not 0 <= g < fields.n_goals:
                continue
            if lookahead is not None:
                way[e, k], hops[e, k] = seed_rule.waypoint(worlds[g], points[e, k], lookahead, tables[g])
            if max_points is not None:
                paths[e, k], counts[e, k] = seed_rule.path(worlds[g], points[e, k], max_points, tables[g])
    return (way, hops) if max_points is None else (paths, counts)


def _equal(got, want):
    got = _np(got)
    return np.array_equal(bits(got), bits(want)) if got.dtype == np.float32 else np.array_equal(got, want)


def test_seeded_waypoints_and_paths_are_the_rules_bits():
    from megastep_amd import cuda
    w = _nine()
    grid, maps = w['grid'], _first_maps(w)
    rng = np.random.RandomState(17)
    points = _points(w['core'].scenery, w['geoms'], rng, spread=24, spawn=24)
    which = rng.randint(0, 2, points.shape[:2]).astype(np.int32)
    which[:, 5::11] = [[2, -1, 7, -3]]                               # no such field
    pts, goal = torch.as_tensor(points, device='cuda'), torch.as_tensor(which, device='cuda')
    on_seed = ahead = none = cut = 0
    for fields in (maps.frontier_fields(), cuda.seeded_fields(grid, maps.values, 2, where=True)):
        way, hops = fields.waypoints(pts, goal=goal, hops=True)
        found = fields.paths(pts, goal=goal, max_points=24)
        want_way, want_hops = _follow_rule(grid, fields, points, which, lookahead=16)
        want_paths, want_counts = _follow_rule(grid, fields, points, which, max_points=24)
        assert _equal(hops, want_hops) and _equal(way, want_way)
        assert _equal(found.counts, want_counts) and _equal(found.points, want_paths)
        # no path: exactly where the query says +inf, a field index out of range included
        assert torch.equal(hops < 0, torch.isinf(fields.at(pts, goal=goal))) and torch.equal(hops < 0, found.counts == 0)
        assert torch.equal(torch.isnan(way).any(-1), hops < 0) and (hops[:, 5::11] == -1).all()
        assert (want_hops >= 0).sum() >= .3*want_hops.size and (want_counts >= 0).all()
        on_seed, ahead, none, cut = on_seed + (want_hops == 0).sum(), ahead + (want_hops >= 2).sum(), none + (want_counts == 0).sum(), cut + (want_counts > 24).sum()
        for L in (1, 64):
            way, hops = fields.waypoints(pts, goal=goal, lookahead=L, hops=True)
            want_way, want_hops = _follow_rule(grid, fields, points, which, lookahead=L)
            assert _equal(hops, want_hops) and _equal(way, want_way), L
    assert on_seed > 0 and ahead > 0 and none > 0 and cut > 0, (on_seed, ahead, none, cut)    # (cut: longer than was written)
    # point k against field k, when there is one point per field
    two = pts[:, -2:].contiguous()
    own = torch.tensor([[0, 1]]*9, device='cuda')
    assert torch.equal(fields.waypoints(two).view(torch.int32), fields.waypoints(two, goal=own).view(torch.int32))
    assert torch.equal(fields.paths(two, max_points=4).counts, fields.paths(two, goal=own, max_points=4).counts)


def test_seeing_more_never_brings_the_frontier_nearer():
    w = _nine()
    maps = _first_maps(w)
    frontier = maps.frontier_fields()
    values, seeds = frontier.values.clone(), frontier.n_seeds.clone()
    _second_frame(w, maps)
    assert (maps.values != w['first']).any()
    assert frontier.update() is frontier
    assert (frontier.n_seeds <= seeds).all() and (frontier.n_seeds < seeds).any()
    assert (frontier.values >= values).all() and (frontier.values > values).any()
    want, counts = _rule_fields(w['grid'], maps.values, 2, 0, maps.countable)
    assert np.array_equal(_np(frontier.n_seeds), counts)
    _fields_equal(w['grid'], frontier, want)


def test_mask_out_a_side_stream_and_a_graph_replayed_three_times():
    from megastep_amd import cuda
    w = _nine()
    grid, maps = w['grid'], _first_maps(w)
    whole = maps.frontier_fields()
    rng = np.random.RandomState(4)
    mask = torch.as_tensor(rng.rand(9, 2) < .5, device='cuda')
    assert mask.any() and not mask.all()
    # without out: fields never computed are +inf
    some = maps.frontier_fields(mask=mask)
    for e in range(9):
        for g in range(2):
            if mask[e, g]:
                assert torch.equal(some.image(e, g).view(torch.int32), whole.image(e, g).view(torch.int32))
            else:
                assert torch.isinf(some.image(e, g)).all() and int(some.n_seeds[e, g]) == 0
    # with out: unmarked fields keep their bytes
    before, seeds = whole.values.clone(), whole.n_seeds.clone()
    _second_frame(w, maps)
    assert maps.frontier_fields(mask=mask, out=whole) is whole
    fresh = maps.frontier_fields()
    for e in range(9):
        first, ny, nx = grid.cells(e)
        for g in range(2):
            at = slice(2*first + g*ny*nx, 2*first + (g + 1)*ny*nx)
            marked = bool(mask[e, g])
            assert torch.equal(whole.values[at].view(torch.int32), (fresh.values if marked else before)[at].view(torch.int32)), (e, g)
            assert int(whole.n_seeds[e, g]) == int((fresh.n_seeds if marked else seeds)[e, g])
    assert not torch.equal(before.view(torch.int32), fresh.values.view(torch.int32))
    with pytest.raises(RuntimeError, match='`out`'):
        cuda.seeded_fields(grid, maps.values, 2, where=True, out=whole)
    with pytest.raises(RuntimeError, match='mask'):
        whole.update(mask.int())
    # a side stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        there = maps.frontier_fields()
    side.synchronize()
    assert torch.equal(there.values.view(torch.int32), fresh.values.view(torch.int32)) and torch.equal(there.n_seeds, fresh.n_seeds)
    # captured once, replayed three times on marks, masks and points changed in place
    pts = torch.as_tensor(_points(w['core'].scenery, w['geoms'], rng, spread=0, spawn=2), device='cuda')
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        whole.update(mask); whole.waypoints(pts, hops=True)
    torch.cuda.current_stream().wait_stream(side)
    with torch.cuda.graph(graph):
        whole.update(mask)
        way, hops = whole.waypoints(pts, hops=True)
    other = _first_maps(w)
    _second_frame(w, other)
    marks = (w['first'], other.values, torch.zeros_like(w['first']))     # one frame, two, nothing seen yet
    for trial in range(3):
        maps.values.copy_(marks[trial])
        mask.copy_(torch.as_tensor(rng.rand(9, 2) < .6, device='cuda'))
        pts.copy_(torch.as_tensor(_points(w['core'].scenery, w['geoms'], rng, spread=0, spawn=2), device='cuda'))
        held = whole.values.clone()
        graph.replay()
        eager = maps.frontier_fields()
        want = torch.where(_cells_of(grid, mask), eager.values, held)
        assert torch.equal(whole.values.view(torch.int32), want.view(torch.int32)), trial
        want_way, want_hops = whole.waypoints(pts, hops=True)
        assert torch.equal(way.view(torch.int32), want_way.view(torch.int32)) and torch.equal(hops, want_hops)
        assert (hops >= 0).any()


def _cells_of(grid, mask):
    """The (N, G) mask of fields, spread over the fields' flat store: a bool per value."""
    out = torch.zeros(max(mask.shape[1]*grid.n_cells, 1), dtype=torch.bool, device=mask.device)
    for e in range(grid.n_envs):
        first, ny, nx = grid.cells(e)
        for g in range(mask.shape[1]):
            out[mask.shape[1]*first + g*ny*nx:mask.shape[1]*first + (g + 1)*ny*nx] = mask[e, g]
    return out


def test_frontiers_follow_the_maps_and_a_shared_map_has_one_field():
    from megastep_amd import cuda, modules
    w = _nine()
    c, grid = w['core'], w['grid']
    for shared in (False, True):
        cover = modules.Coverage(c, grid, max_range=4., shared=shared, countable=w['maps'].countable)
        cover(modules.render(c, fields=('distances',)))
        frontiers = modules.Frontiers(c, cover, refresh=4)
        assert frontiers.fields.n_goals == (1 if shared else 2)
        way, d = frontiers.waypoints(), frontiers.distance()
        assert way.shape == (9, 2, 2) and d.shape == (9, 2) and torch.equal(torch.isnan(way).any(-1), torch.isinf(d))
        field = torch.zeros((9, 2), dtype=torch.int64, device='cuda') if shared else None
        assert torch.equal(d, cover.maps.frontier_fields().at(c.agents.positions, goal=field))
        # step 0: everything is due; steps 1 and 2: nothing is; step 3: an agent that starts over, at once; step 4: everything
        frontiers()
        _second_frame(w, cover=cover)
        held = frontiers.fields.values.clone()
        frontiers(); frontiers()
        assert torch.equal(frontiers.fields.values.view(torch.int32), held.view(torch.int32))
        reset = torch.zeros((9, 2), dtype=torch.bool, device='cuda')
        reset[4, 1] = True
        frontiers(reset)
        fresh = cover.maps.frontier_fields()
        first, ny, nx = grid.cells(4)
        G = frontiers.fields.n_goals
        mine = slice(G*first + (G - 1)*ny*nx, G*first + G*ny*nx)
        assert torch.equal(frontiers.fields.values[mine].view(torch.int32), fresh.values[mine].view(torch.int32))
        assert torch.equal(frontiers.fields.values[:G*first].view(torch.int32), held[:G*first].view(torch.int32))
        frontiers()                                                     # (env 4's agent 1 is at its step 1 now: computed last step, from these marks)
        assert torch.equal(frontiers.fields.values.view(torch.int32), fresh.values.view(torch.int32))
        assert not torch.equal(held.view(torch.int32), fresh.values.view(torch.int32))


def _rollout(env, steps, policy, seed=1):
    """`steps` steps under env.expert() or uniformly random actions. Returns (episodes that ended by coverage, episodes that
    ended by lifespan, the mean over all episodes - those still running at the end included - of the fraction seen at their
    last step)."""
    from megastep_amd import arrdict
    rng = np.random.RandomState(seed)
    n, a = env.core.n_envs, env.core.n_agents
    env.reset()
    by_coverage = by_lifespan = 0
    final = []
    for t in range(steps):
        fraction = env._coverage.fraction().clone()
        over = env._over.clone()                                         # who starts over at this step: their episode ended at the last
        done = fraction >= env.complete
        by_coverage += int((over & done).sum())
        by_lifespan += int((over & ~done).sum())
        final += fraction[over].tolist()
        decision = env.expert() if policy == 'expert' else arrdict.arrdict(actions=torch.as_tensor(rng.randint(0, 7, (n, a)), device='cuda'))
        env.step(decision)
    final += env._coverage.fraction().reshape(-1).tolist()
    return by_coverage, by_lifespan, float(np.mean(final))


def test_the_expert_sees_the_floor_at_least_as_often_as_a_random_policy():
    """FloorCoverage(64), 300 steps, once under env.expert() and once under uniformly random actions, the same seeds: the expert
    ends episodes by coverage, at least as many as the random policy, and its mean final fraction is not below the random
    policy's."""
    from megastep_amd.demo import FloorCoverage
    results = {}
    for policy in ('expert', 'random'):
        torch.manual_seed(3); np.random.seed(3)
        env = FloorCoverage(64, geometries=plans(64), max_lifespan=300)
        results[policy] = _rollout(env, 300, policy)
        print(f'FloorCoverage(64), 300 steps, {policy}: {results[policy][0]} episodes ended by coverage, {results[policy][1]} by lifespan, '
              f'mean final fraction {results[policy][2]:.3f}')
        if policy == 'expert':
            actions = env.expert().actions
            assert actions.shape == (64, 1) and actions.dtype == torch.int64 and ((actions >= 0) & (actions < 7)).all()
    expert, random = results['expert'], results['random']
    assert expert[0] > 0 and expert[0] >= random[0] and expert[2] >= random[2], results


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
    from megastep_amd.demo import FloorCoverage
    logs = []
    for graphed in (False, True):
        torch.manual_seed(3); np.random.seed(3)
        env = FloorCoverage(16, n_agents=2, geometries=plans(16), max_lifespan=10**6, complete=.3)
        stepper = graphs.GraphedStep(_Expert(env), warmup=3) if graphed else _Expert(env)
        stepper.reset()
        nothing = arrdict.arrdict(actions=torch.zeros((16, 2), dtype=torch.long, device='cuda'))
        log = []
        # the graphed env's first step call is four steps: three of warm-up and the captured one
        for t in range(10 if graphed else 13):
            world = stepper.step(nothing)
            log.append((world.reward.clone(), world.reset.clone(), env.maps.values.clone(), env.core.agents.positions.clone()))
        logs.append(log)
    eager, graphed = logs
    for k in range(10):
        for got, want in zip(graphed[k], eager[k + 3]):
            assert torch.equal(got, want), k
    assert sum(float(r.sum()) for r, _, _, _ in graphed) > 0
    assert not torch.equal(graphed[0][3], graphed[-1][3])                # (they moved)
