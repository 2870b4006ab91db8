"""Flow fields on the GPU: nav_flow_kernel and nav_flow_query_kernel (csrc/kernels/navflow.h) held to EQUALITY - integers, and floats
as bits - with flow_rule (tests/flow_rule.py), the numpy statement, on fields read back from the device. The tiers' edges, a byte a
framed cell: 126 x 126 = 16384 fills the 16 KiB instantiation, 254 x 254 the 64 KiB one, 510 x 318 the 160 KiB one; a column more
takes the next, and beyond the last the env's hops come from global memory."""
import numpy as np
import pytest
import torch

from tests.flow_rule import flow_rule
from tests.test_gpu_navseen import _by_hand, _np, _six
from tests.test_navcost_host import cost_rule
from tests.test_navfield_host import CELL, F, RADIUS, bits, plans
from tests.test_navflow_host import FREE, GEOM, _points
from tests.test_navpath_host import NAN, path_rule
from tests.test_navseed_host import seed_rule

pytestmark = pytest.mark.gpu

# (the grid: the six plans, the hand-made plan, or a (tier, nx, ny) at a tier's edge; kind; fields an env; L; points an env)
CASES = ([('six', kind, 2, 16, 70) for kind in ('goal', 'seeded', 'cost')] + [('hand', 'goal', P, 8, P) for P in (1, 64, 65, 257)]
         + [(edge, kind, 2, L, 9) for edge in ((0, 126, 126), (0, 127, 126), (1, 254, 254), (1, 255, 254), (2, 510, 318), (2, 511, 318))
            for kind, L in (('goal', 16), ('seeded', 64))])


def _grid(what, rng):
    from megastep_amd import cuda
    if isinstance(what, str):
        return cuda.nav_grid(_six()['core'].scenery, clearance=RADIUS) if what == 'six' else _by_hand([(GEOM, FREE)])
    tier, nx, ny = what
    grid = _by_hand([((-37, -52, nx, ny), rng.rand(ny, nx) < .8), ((3, -4, 9, 7), rng.rand(7, 9) < .8), ((-2, 5, 1, 300), rng.rand(300, 1) < .97),
                     ((0, 0, 5, 5), np.zeros((5, 5), bool)), ((0, 0, 0, 0), np.zeros((0, 0), bool))])
    cap = cuda.FLOW_CAPACITY[tier]
    assert grid._max_framed == (nx + 2)*(ny + 2) and (grid._max_framed == cap or cap < grid._max_framed <= cap + ny + 2)
    return grid


def _near(envs, rng, count):
    """(N, count, 2): points within half a cell of free cells' centres; zeros in an env that has none."""
    return np.array([_points(env, rng, count) if env[2].any() else np.zeros((count, 2), F) for env in envs], F)


def _rule(env, start, fields, flows, goals, costs, e, g, rng):
    """(world, table, targets) of field g of env e as the device holds them; with `rng` the targets are held to flow_rule's: on every
    live cell of a small env, on 600 random ones and the last row and column of a large one, and to -1 on every cell that is not live."""
    ny, nx = env[2].shape
    world = env + (_np(fields.image(e, g)).copy(), None if goals is None else goals[e, g])
    table = path_rule.hops(world) if goals is not None else seed_rule.hops(world[:4]) if costs is None else cost_rule.hops(world[:4], costs[start:start + ny*nx].reshape(ny, nx))
    live, got = flow_rule.live(world), _np(flows.image(e, g))
    cells = np.argwhere(live)
    if rng and len(cells) > 600:
        cells = np.concatenate([cells[(cells[:, 0] == ny - 1) | (cells[:, 1] == nx - 1)], cells[rng.choice(len(cells), 600, replace=False)]])
    asked, want = ~live, flow_rule.targets(world, table, flows.lookahead, cells if rng else cells[:0])
    asked[tuple(cells.T)] = rng is not None
    assert np.array_equal(got[asked], want[asked]), (e, g, np.argwhere(asked & (got != want))[:5].tolist())
    return world, table, got


@pytest.mark.parametrize('what,kind,G,L,P', CASES, ids=lambda v: 'x'.join(map(str, v[1:])) if isinstance(v, tuple) else str(v))
def test_targets_and_answers_are_the_rules(what, kind, G, L, P):
    from megastep_amd import cuda
    rng, dev = np.random.RandomState(G + P), lambda a: torch.as_tensor(a, device='cuda')
    grid = _grid(what, rng)
    envs = [(tuple(map(int, g)), grid.cell, _np(grid.free)[s:s + g[2]*g[3]].reshape(g[3], g[2]) != 0) for g, s in zip(_np(grid.geom), _np(grid.starts))]
    marks = dev((rng.rand(max(G*grid.n_cells, 1)) < .002).astype(np.uint8))
    goals = _near(envs, rng, G) if kind == 'goal' else None
    costs = (1 + 5*(rng.rand(grid.free.shape[0]) < .3)).astype(F) if kind == 'cost' else None
    fields = cuda.distance_fields(grid, dev(goals)) if kind == 'goal' else cuda.seeded_fields(grid, marks, G) if kind == 'seeded' else cuda.cost_fields(grid, marks, G, dev(costs))
    flows = fields.flows(lookahead=L)
    rules = {(e, g): _rule(env, int(grid.starts[e]), fields, flows, goals, costs, e, g, rng if g in (0, G - 1) else None)
             for e, env in enumerate(envs) if env[2].size for g in range(G)}
    # the query: points round free cells, two that have no anchor; among the fields asked, -1 and G
    points, given = _near(envs, rng, P), rng.randint(0, G, (len(envs), P)).astype(np.int32)
    if P > 2:
        points[:, 0], points[:, 1, 0], given[:, 2], given[:, 3] = np.nan, 1e9, -1, G
    for goal in [given] + [None]*(P == G):
        way, took = (_np(t) for t in (flows.at(dev(points), goal=None if goal is None else dev(goal), took=True), flows.took))
        for e, k in [(e, k) for e in range(len(envs)) for k in range(P)]:
            g = k if goal is None else goal[e, k]
            want = flow_rule.at(*rules[e, g], points[e, k]) if (e, g) in rules else ((NAN, NAN), -1)
            assert np.array_equal(bits(way[e, k]), bits(np.array(want[0], F))) and took[e, k] == want[1], (e, k, g)
    assert (took >= 0).any() and (what != 'six' or ((took == 1).sum() > 100 and (took == 0).any()))


def test_update_update_at_on_a_side_stream_and_as_a_graph_replayed_over_new_goals_give_the_eager_results():
    from megastep_amd import cuda
    grid, rng = _grid('hand', None), np.random.RandomState(8)
    near = lambda: torch.as_tensor(_points((GEOM, CELL, FREE), rng, 3)[None], device='cuda')
    points, new_goals, mask = near(), near(), torch.ones((1, 3), dtype=torch.bool, device='cuda')
    fields = cuda.distance_fields(grid, near())
    flows, out = fields.flows(), torch.empty_like(points)
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fields.update(new_goals, mask=mask); flows.update(mask=mask); flows.at(points, out=out, took=True)
    torch.cuda.current_stream().wait_stream(side)
    with torch.cuda.graph(graph):
        fields.update(new_goals, mask=mask); flows.update(mask=mask); flows.at(points, out=out, took=True)
    for replay in range(4):                                              # (0: what the side stream left)
        if replay:
            new_goals.copy_(near())
            graph.replay()
        fresh = cuda.distance_fields(grid, new_goals).flows()
        want = fresh.at(points, took=True)
        assert torch.equal(flows.targets, fresh.targets) and torch.equal(out.view(torch.int32), want.view(torch.int32)) and torch.equal(flows.took, fresh.took), replay


def test_a_crowd_that_flows_ticks_in_a_graph_as_it_does_eagerly():
    """(Without `flow` a Crowd is the parent's, whose ticks tests/test_gpu_walkers.py holds to their rule; here only the default is guarded.)"""
    from megastep_amd import arrdict, graphs
    from megastep_amd.demo import Crowd
    assert Crowd(16, n_walkers=12, geometries=plans(16)).walkers.flows is None
    logs = {}
    for graphed in (False, True):
        torch.manual_seed(3); np.random.seed(3)
        env = Crowd(16, n_walkers=12, geometries=plans(16), max_lifespan=10**6, flow=True)
        stepper = graphs.GraphedStep(env, warmup=3) if graphed else env
        stepper.reset()
        for t in (range(6) if graphed else [0, 0, 0] + list(range(6))):
            actions = torch.as_tensor(np.random.RandomState(100 + t).choice([1, 3, 5], (16, 1)), device='cuda')
            world = stepper.step(arrdict.arrdict(actions=actions))
            logs.setdefault(graphed, []).append([bits(_np(x)).copy() for x in (world.obs.rgb, world.obs.d, world.reward, env.walkers.positions, env.walkers.store.velocities)])
    assert env.walkers.flows is not None and all(np.array_equal(x, y) for s, t in zip(logs[False][3:], logs[True]) for x, y in zip(s, t))
    first, last = (logs[False][t][3].view(F) for t in (0, -1))
    assert np.isfinite(last).all() and np.abs(last - first).max() > .1
