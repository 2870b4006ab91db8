"""Pulled paths on the GPU: `DistanceFields.pulled`, `SeededFields.pulled` and `CostFields.pulled` equal AS BITS to the numpy
statement of the contract (tests/test_navpull_host.pull_rule) on the fields the kernels themselves computed - vertices, indices,
counts, cells and lengths; either of the wave's two sight schemes; masks, `out=`, streams and graph capture; the hand-made grids
of the CPU suite on the device; and `PointGoal(spl=True)`, eager and as one HIP graph."""
import numpy as np
import pytest
import torch

from tests.test_navfield_host import CELL, RADIUS, F, bits, plans
from tests.test_navpath_host import path_rule
from tests.test_navseed_host import seed_rule
from tests.test_navcost_host import cost_rule
from tests.test_navpull_host import CORRIDORS, constant, corner, corridor, pull_rule, room, seeded_on_a_seed
from tests.test_gpu_navfield import _draw_goals, _scenery
from tests.test_gpu_navpath import _Expert, _points, _worlds
from tests.test_gpu_navseen import _np
from tests.test_gpu_navseed import _env, _first_maps, _nine
from tests.test_gpu_navcost import _cost_of, _three

pytestmark = pytest.mark.gpu

REACHES = (1, 63, 64, 65, 256)


def _tables(grid, fields, e):
    """The rule's worlds, hop tables and chain of env e's fields - read back from the device - whatever their kind."""
    from megastep_amd import cuda
    if isinstance(fields, cuda.DistanceFields):
        worlds, tables = _worlds(grid, fields, e)
        return worlds, tables, path_rule.chain
    geom, free, _ = _env(grid, e)
    worlds = [(geom, CELL, free, _np(fields.image(e, g))) for g in range(fields.n_goals)]
    if isinstance(fields, cuda.CostFields):
        return worlds, [cost_rule.hops(w, _cost_of(fields, e, g)) for g, w in enumerate(worlds)], cost_rule.chain
    return worlds, [seed_rule.hops(w) for w in worlds], seed_rule.chain


def _rule(grid, fields, points, which, reach):
    """pull_rule's answer for points (N, P, 2) following fields `which` (N, P): [env][point] a pull, None without a path."""
    found = []
    for e in range(points.shape[0]):
        worlds, tables, chain = _tables(grid, fields, e)
        found.append([pull_rule.pull(worlds[g], points[e, k], reach, tables[g], chain) if 0 <= g < fields.n_goals else None
                      for k, g in enumerate(int(g) for g in which[e])])
    return found


def _outputs(found, max_points):
    """The five outputs of a whole call, from _rule's pulls."""
    rows = [[pull_rule.outputs(pulled, max_points) for pulled in env] for env in found]
    stack = lambda k, dtype: np.array([[row[k] for row in env] for env in rows], dtype)
    return stack(0, F), stack(1, np.int32), stack(2, np.int32), stack(3, np.int32), stack(4, F)


def _equal(got, want):
    got = _np(got)
    return np.array_equal(bits(got), bits(want)) if got.dtype == np.float32 else np.array_equal(got, want)


def _holds(pulled, want):
    vertices, indices, counts, cells, lengths = want
    assert _equal(pulled.counts, counts), (_np(pulled.counts), counts)
    assert _equal(pulled.cells, cells)
    assert _equal(pulled.points, vertices) and _equal(pulled.indices, indices)
    assert _equal(pulled.lengths, lengths), (_np(pulled.lengths), lengths)


def _compare(grid, fields, points, which, reaches=REACHES, max_points=(2, 64)):
    """The kernel against the rule at every reach and max_points; returns the rule's (counts, cells) at the last reach."""
    pts, goal = torch.as_tensor(points, device='cuda'), torch.as_tensor(which, device='cuda')
    for reach in reaches:
        found = _rule(grid, fields, points, which, reach)
        for M in max_points:
            want = _outputs(found, M)
            _holds(fields.pulled(pts, goal=goal, reach=reach, max_points=M, indices=True), want)
    plain = fields.pulled(pts, goal=goal, reach=reaches[-1], max_points=max_points[-1])
    assert plain.indices is None and _equal(plain.points, want[0]) and _equal(plain.lengths, want[4])
    return want[2], want[3]


def _by_sample(fields, pts, goal, reach, max_points):
    """The same call under the waypoint kernel's sight scheme, a lane a sample."""
    from megastep_amd import _lib
    assert _lib.lib().ms_debug_nav_pull_scheme(1) == 0
    try:
        return fields.pulled(pts, goal=goal, reach=reach, max_points=max_points, indices=True)
    finally:
        assert _lib.lib().ms_debug_nav_pull_scheme(-1) == 0


def _same_bits(a, b):
    for name in ('points', 'indices', 'counts', 'cells', 'lengths'):
        x, y = getattr(a, name), getattr(b, name)
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), name


# ---------------------------------------------------------------------------------------------------------------------
# 1. the kernel is the rule, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('oblique', [False, True])
def test_pulled_paths_are_the_rules_bits(oblique):
    from megastep_amd import cuda
    geoms = plans(4, oblique)
    sc = _scenery(geoms)
    rng = np.random.RandomState(31 + oblique)
    grid = cuda.nav_grid(sc, clearance=RADIUS)
    fields = cuda.distance_fields(grid, torch.as_tensor(_draw_goals(geoms, 2, rng), device='cuda'))
    points = _points(sc, geoms, rng, spread=16, spawn=16)
    which = rng.randint(0, 2, points.shape[:2]).astype(np.int32)
    which[:, 5::11] = [[2, -1, 7]]                                       # no such field
    counts, cells = _compare(grid, fields, points, which)
    # the equality is not one of empty answers: most spawn points have a path, some chains outrun a window, some paths M = 64... and
    # no path exactly where the query says +inf
    pts, goal = torch.as_tensor(points, device='cuda'), torch.as_tensor(which, device='cuda')
    assert (counts[:, 16:] > 0).sum() >= .7*counts[:, 16:].size and (cells > 65).any() and (counts == 0).any() and (counts >= 0).all()
    pulled = fields.pulled(pts, goal=goal, reach=64)
    assert torch.equal(pulled.counts == 0, torch.isinf(fields.at(pts, goal=goal))) and torch.equal(pulled.counts == 0, torch.isinf(pulled.lengths))
    assert (pulled.counts[:, 5::11] == 0).all() and torch.isnan(pulled.points[:, 5::11]).all()
    e, k = np.argwhere(counts > 2)[0]
    assert pulled.path(e, k).shape == (min(int(pulled.counts[e, k]), 64), 2)
    # pulled <= the field's own (octile) distance, up to the roundings of either sum
    at, L = _np(fields.at(pts, goal=goal)), _np(pulled.lengths)
    there = np.isfinite(at)
    assert (L[there] <= at[there]*(1 + 1e-5)).all() and (L[there] < at[there]*.99).sum() > .5*there.sum()
    # either sight scheme, the same bits
    for reach in (64, 256):
        _same_bits(_by_sample(fields, pts, goal, reach, 64), fields.pulled(pts, goal=goal, reach=reach, max_points=64, indices=True))


def test_a_large_plan_with_chains_of_hundreds_of_cells():
    from megastep_amd import cuda
    geoms = plans(1, large=True)
    sc = _scenery(geoms)
    rng = np.random.RandomState(18)
    grid = cuda.nav_grid(sc, clearance=RADIUS)
    fields = cuda.distance_fields(grid, torch.as_tensor(_draw_goals(geoms, 2, rng), device='cuda'))
    points = _points(sc, geoms, rng, spread=8, spawn=24)
    which = rng.randint(0, 2, points.shape[:2]).astype(np.int32)
    counts, cells = _compare(grid, fields, points, which, reaches=(1, 16, 64), max_points=(2, 16))
    print(f'the longest chain has {cells.max()} points; at reach 64 the paths have up to {counts.max()} vertices')
    assert cells.max() > 100 and (cells > 4*16).sum() > 8 and (cells > 64).sum() > 8 and counts.max() > 16
    pts, goal = torch.as_tensor(points, device='cuda'), torch.as_tensor(which, device='cuda')
    _same_bits(_by_sample(fields, pts, goal, 64, 16), fields.pulled(pts, goal=goal, reach=64, max_points=16, indices=True))


def test_pulled_paths_on_seeded_fields_are_the_rules_bits():
    w = _nine()
    grid, maps = w['grid'], _first_maps(w)
    rng = np.random.RandomState(37)
    points = _points(w['core'].scenery, w['geoms'], rng, spread=4, spawn=8)
    which = rng.randint(0, 2, points.shape[:2]).astype(np.int32)
    which[:, 5] = 2
    counts, cells = _compare(grid, maps.frontier_fields(), points, which)
    assert (counts > 0).sum() >= .3*counts.size and (counts >= 0).all() and (counts[:, 5] == 0).all()
    assert (cells == 2).any() or (cells > 8).any()


@pytest.mark.parametrize('n_costs', [1, 2])
def test_pulled_paths_on_cost_fields_are_the_rules_bits(n_costs):
    from megastep_amd import cuda
    w = _three()
    grid = w['grid']
    fields = cuda.cost_fields(grid, w['marks'], 2, w['shared'] if n_costs == 1 else w['own'])
    rng = np.random.RandomState(41 + n_costs)
    points = _points(w['core'].scenery, w['geoms'], rng, spread=8, spawn=16)
    which = rng.randint(0, 2, points.shape[:2]).astype(np.int32)
    which[:, 5] = -1
    counts, cells = _compare(grid, fields, points, which)
    assert (counts > 0).sum() >= .3*counts.size and (counts >= 0).all() and (cells > 8).any()
    # the weighted hop is not the unweighted one: the seeded pull on the same values goes another way somewhere
    pts, goal = torch.as_tensor(points, device='cuda'), torch.as_tensor(which, device='cuda')
    seeded = cuda.SeededFields(grid, fields.marks, 2, True, None, fields.values, fields.n_seeds)
    plain, priced = seeded.pulled(pts, goal=goal, reach=64), fields.pulled(pts, goal=goal, reach=64)
    assert not torch.equal(plain.points.view(torch.int32), priced.points.view(torch.int32))


def test_goal_indices_a_second_agent_and_a_side_stream():
    from megastep_amd import cuda
    geoms = plans(4)
    sc = _scenery(geoms, n_agents=2)
    rng = np.random.RandomState(19)
    grid = cuda.nav_grid(sc, clearance=RADIUS)
    fields = cuda.distance_fields(grid, torch.as_tensor(_draw_goals(geoms, 2, rng), device='cuda'))
    points = _points(sc, geoms, rng, spread=0, spawn=2)                  # two agents an env, each with a field of its own
    pts = torch.as_tensor(points, device='cuda')
    own = np.array([[0, 1]]*4, np.int32)
    want = _outputs(_rule(grid, fields, points, own, 64), 16)
    mine = fields.pulled(pts, reach=64, max_points=16, indices=True)
    _holds(mine, want)
    assert (want[2] > 0).sum() >= 6
    _same_bits(mine, fields.pulled(pts, goal=torch.as_tensor(own, device='cuda'), reach=64, max_points=16, indices=True))
    swapped = fields.pulled(pts, goal=torch.as_tensor(1 - own, device='cuda').long(), reach=64, max_points=16, indices=True)
    _holds(swapped, _outputs(_rule(grid, fields, points, 1 - own, 64), 16))
    assert not torch.equal(swapped.points.view(torch.int32), mine.points.view(torch.int32))
    seven = fields.pulled(pts, goal=torch.full((4, 2), 7, dtype=torch.int64, device='cuda'), max_points=4, indices=True)
    assert (seven.counts == 0).all() and (seven.cells == 0).all() and torch.isnan(seven.points).all() and (seven.indices == -1).all()
    assert torch.isinf(seven.lengths).all() and (seven.lengths > 0).all()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        there = fields.pulled(pts, reach=64, max_points=16, indices=True)
    side.synchronize()
    _same_bits(there, mine)


# ---------------------------------------------------------------------------------------------------------------------
# 2. masks and out=
# ---------------------------------------------------------------------------------------------------------------------
def test_a_mask_keeps_the_unmarked_rows_and_out_is_rewritten_in_place():
    from megastep_amd import cuda
    geoms = plans(4)
    sc = _scenery(geoms)
    rng = np.random.RandomState(43)
    grid = cuda.nav_grid(sc, clearance=RADIUS)
    fields = cuda.distance_fields(grid, torch.as_tensor(_draw_goals(geoms, 2, rng), device='cuda'))
    points = _points(sc, geoms, rng, spread=4, spawn=12)
    which = rng.randint(0, 2, points.shape[:2]).astype(np.int32)
    pts, goal = torch.as_tensor(points, device='cuda'), torch.as_tensor(which, device='cuda')
    full = fields.pulled(pts, goal=goal, reach=64, max_points=8, indices=True)
    mask = torch.as_tensor(rng.rand(4, 16) < .5, device='cuda')
    held = cuda.PulledPaths(torch.full((4, 16, 8, 2), -5., device='cuda'), torch.full((4, 16), -5, dtype=torch.int32, device='cuda'),
                            torch.full((4, 16), -5., device='cuda'), torch.full((4, 16), -5, dtype=torch.int32, device='cuda'),
                            torch.full((4, 16, 8), -5, dtype=torch.int32, device='cuda'))
    tensors = [getattr(held, name) for name in ('points', 'indices', 'counts', 'cells', 'lengths')]
    where = [t.data_ptr() for t in tensors]
    assert fields.pulled(pts, goal=goal, reach=64, max_points=8, indices=True, mask=mask, out=held) is held
    assert [t.data_ptr() for t in tensors] == where
    assert mask.any() and not mask.all()
    for name in ('points', 'indices', 'counts', 'cells', 'lengths'):
        got, want = getattr(held, name), getattr(full, name)
        assert torch.equal(got[mask].view(torch.int32), want[mask].view(torch.int32)), name
        assert (got[~mask] == -5).all(), name
    # ... and the rest on a second call
    fields.pulled(pts, goal=goal, reach=64, max_points=8, indices=True, mask=~mask, out=held)
    _same_bits(held, full)
    # a fresh result under a mask holds "no path" where nothing was pulled
    fresh = fields.pulled(pts, goal=goal, reach=64, max_points=8, mask=mask)
    assert (fresh.counts[~mask] == 0).all() and torch.isinf(fresh.lengths[~mask]).all() and torch.isnan(fresh.points[~mask]).all()
    with pytest.raises(RuntimeError, match='out'):
        fields.pulled(pts, goal=goal, max_points=16, out=held)
    with pytest.raises(RuntimeError, match='mask'):
        fields.pulled(pts, goal=goal, mask=mask[:, :8])


# ---------------------------------------------------------------------------------------------------------------------
# 3. the hand-made grids of the CPU suite
# ---------------------------------------------------------------------------------------------------------------------
def _grid_of(worlds):
    """A NavGrid whose envs are the hand-made worlds' grids, as they stand."""
    from megastep_amd import cuda
    geom = np.array([w[0] for w in worlds], np.int32)
    starts = np.concatenate([[0], np.cumsum([w[2].size for w in worlds])]).astype(np.int64)
    free = np.concatenate([w[2].reshape(-1) for w in worlds]).astype(np.uint8)
    return cuda.NavGrid(torch.as_tensor(geom, device='cuda'), torch.as_tensor(starts, device='cuda'), torch.as_tensor(free, device='cuda'),
                        CELL, RADIUS, geom, starts)


def test_hand_made_grids_on_the_device():
    from megastep_amd import cuda
    made = [room(), corner(), constant()] + [corridor(n) for n in CORRIDORS]
    worlds, starts = [m[0] for m in made], np.array([[m[1]] for m in made], F)
    grid = _grid_of(worlds)
    fields = cuda.distance_fields(grid, torch.as_tensor(np.array([[w[4]] for w in worlds], F), device='cuda'))
    first, ny, nx = grid.cells(2)
    fields.values[first:first + ny*nx] = torch.as_tensor(worlds[2][3].reshape(-1), device='cuda')   # the constant field
    for e, w in enumerate(worlds):                                       # the device's fields are the rule's: the worlds are the CPU suite's
        assert np.array_equal(bits(_np(fields.image(e))), bits(w[3])), e
    zero = np.zeros((len(made), 1), np.int32)
    counts, cells = _compare(grid, fields, starts, zero, reaches=(1, 64), max_points=(2, 8))
    assert cells[:, 0].tolist()[2:] == [-2] + list(CORRIDORS) and counts[:3, 0].tolist() == [2, 3, -2]
    assert counts[3:, 0].tolist() == [len(range(0, n - 1, 64)) + 1 for n in CORRIDORS]
    pts = torch.as_tensor(starts, device='cuda')
    for reach in (1, 64, 1024):
        _same_bits(_by_sample(fields, pts, None, reach, 8), fields.pulled(pts, reach=reach, max_points=8, indices=True))
    got = fields.pulled(pts, reach=64, max_points=8)
    assert torch.equal(got.points[0, 0, :2].view(torch.int32), torch.as_tensor(np.array([starts[0, 0], worlds[0][4]]), device='cuda').view(torch.int32))
    # a start on a seed
    world, p = seeded_on_a_seed()
    grid = _grid_of([world])
    seeded = cuda.SeededFields(grid, torch.zeros(64, dtype=torch.uint8, device='cuda'), 1, True, None,
                               torch.as_tensor(world[3].reshape(-1), device='cuda'), torch.ones((1, 1), dtype=torch.int32, device='cuda'))
    counts, cells = _compare(grid, seeded, np.array([[p]], F), np.zeros((1, 1), np.int32), reaches=(1, 64), max_points=(2, 8))
    assert counts.tolist() == [[2]] and cells.tolist() == [[2]]


# ---------------------------------------------------------------------------------------------------------------------
# 4. graph capture
# ---------------------------------------------------------------------------------------------------------------------
def test_a_captured_call_follows_points_and_fields_changed_in_place():
    from megastep_amd import cuda
    geoms = plans(4)
    sc = _scenery(geoms)
    rng = np.random.RandomState(23)
    grid = cuda.nav_grid(sc, clearance=RADIUS)
    goals = torch.as_tensor(_draw_goals(geoms, 2, rng), device='cuda')
    fields = cuda.distance_fields(grid, goals)
    pts = torch.as_tensor(_points(sc, geoms, rng, spread=0, spawn=2), device='cuda')
    held = fields.pulled(pts, reach=64, max_points=8, indices=True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fields.update(goals); fields.pulled(pts, reach=64, max_points=8, indices=True, out=held)
    torch.cuda.current_stream().wait_stream(side)
    with torch.cuda.graph(graph):
        fields.update(goals)
        fields.pulled(pts, reach=64, max_points=8, indices=True, out=held)
    different, last = 0, None
    for trial in range(3):
        goals.copy_(torch.as_tensor(_draw_goals(geoms, 2, rng), device='cuda'))
        pts.copy_(torch.as_tensor(_points(sc, geoms, rng, spread=0, spawn=2), device='cuda'))
        graph.replay()
        got = [getattr(held, name).clone() for name in ('points', 'indices', 'counts', 'cells', 'lengths')]
        fields.update(goals)                                            # (the same again, eagerly: an update is idempotent)
        want = _outputs(_rule(grid, fields, _np(pts), np.array([[0, 1]]*4), 64), 8)
        assert all(_equal(g, w) for g, w in zip(got, want))
        different += last is not None and not torch.equal(last, got[0].view(torch.int32))
        last = got[0].view(torch.int32).clone()
    assert different == 2 and (got[2] > 0).any()


# ---------------------------------------------------------------------------------------------------------------------
# 5. PointGoal(spl=True)
# ---------------------------------------------------------------------------------------------------------------------
def _spl_log(env, stepper, steps):
    from megastep_amd import arrdict
    world = stepper.reset()
    assert world.spl.shape == (16, 1) and world.spl.dtype == torch.float32
    nothing = arrdict.arrdict(actions=torch.zeros((16, 1), dtype=torch.long, device='cuda'))
    log = []
    for t in range(steps):
        world = stepper.step(nothing)
        log.append(arrdict.arrdict(rgb=world.obs.rgb.clone(), d=world.obs.d.clone(), goal=world.obs.goal.clone(), reset=world.reset.clone(),
                                   reward=world.reward.clone(), spl=world.spl.clone(), over=env._over.clone(),
                                   shortest=env.spl.shortest.clone(), walked=env.spl.walked.clone()))
    return log


def _spl_holds(log):
    """NaN exactly where no episode ended (or no shortest path was there to score it by), within [0, 1] elsewhere; returns
    (episodes scored, those above 0)."""
    ended = scored = 0
    for w in log:
        assert torch.equal(torch.isnan(w.spl), ~(w.over & torch.isfinite(w.shortest)))
        assert (w.shortest >= 0).all() and (w.walked >= 0).all()         # (0: a stranded agent's goal is the spot it stands on)
        there = ~torch.isnan(w.spl)
        assert ((w.spl[there] >= 0) & (w.spl[there] <= 1)).all()
        ended, scored = ended + int(there.sum()), scored + int((w.spl[there] > 0).sum())
    return ended, scored


def test_pointgoal_with_spl_as_one_hip_graph_equals_the_eager_env():
    from megastep_amd import graphs
    from megastep_amd.demo import PointGoal
    geoms = plans(16)
    plain = PointGoal(16, geometries=geoms)
    assert 'spl' not in plain.reset() and plain.spl is None
    logs = []
    for graphed in (False, True):
        torch.manual_seed(3); np.random.seed(3)
        env = PointGoal(16, geometries=geoms, max_lifespan=10**6, arrive=1.5, spl=True)
        stepper = graphs.GraphedStep(_Expert(env), warmup=3) if graphed else _Expert(env)
        logs.append(_spl_log(env, stepper, 40 if graphed else 43))
    eager, graphed = logs
    same = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32)) if a.dtype == torch.float32 else torch.equal(a, b)
    # the graphed env's first step call is four steps (three of warm-up and the captured one): its k-th is the eager env's k + 3
    for k in range(len(graphed)):
        for name in graphed[k]:
            assert same(graphed[k][name], eager[k + 3][name]), (k, name)
    ended, scored = _spl_holds(eager)
    print(f'PointGoal(16, arrive=1.5, spl=True), 43 steps under the expert: {ended} episodes ended, {scored} of them at the goal')
    # episodes that end on their lifespan, every few steps: all score 0 or NaN-free within [0, 1], and everyone is scored
    torch.manual_seed(3); np.random.seed(3)
    env = PointGoal(16, geometries=geoms, max_lifespan=8, spl=True)
    ended, scored = _spl_holds(_spl_log(env, _Expert(env), 20))
    print(f'PointGoal(16, max_lifespan=8, spl=True), 20 steps: {ended} episodes ended, {scored} of them at the goal')
    assert ended >= 32                                                   # (a lifespan is under 8 steps: two episodes an agent at least)
