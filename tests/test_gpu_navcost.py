"""Cost fields on the GPU: `cuda.cost_fields` equal AS BITS to the numpy statement of the contract
(tests/test_navcost_host.cost_rule) - fields, seed counts, passes, queries - with a cost store an env and one a field, both variants
of where the kernel keeps a cell's multiplier, every LDS tier of each variant at its edge and the global-memory path; the reduction
to `cuda.seeded_fields` and the clamp; `waypoints` and `paths` against the rule and the host instantiations; `update()` and a
captured graph after the costs were rewritten in place; and `modules.Routes`, `Frontiers(cost=)` and `PointGoal(margin=)`."""
import ctypes

import numpy as np
import pytest
import torch

from tests.test_navfield_host import CELL, RADIUS, F, bits, nav_rule, plans
from tests.test_navseed_host import seed_rule
from tests.test_navcost_host import clamp_layers, cost_rule, host_cost_follow, inflation
from tests.test_gpu_navseen import _by_hand, _core, _np
from tests.test_gpu_navseed import _env, _equal
from tests.test_gpu_navpath import _points

pytestmark = pytest.mark.gpu

GLOBAL, IN_LDS = 0, 1
SENTINEL = -7.25


class variant:
    """Pins where ms_nav_cost_fields' launch keeps the multipliers, for the calling thread; the library's own choice afterwards."""

    def __init__(self, which):
        self.which = which

    def __enter__(self):
        from megastep_amd import _lib
        assert _lib.lib().ms_debug_nav_cost_variant(self.which) == 0

    def __exit__(self, *exc):
        from megastep_amd import _lib
        _lib.lib().ms_debug_nav_cost_variant(-1)


def _rule_fields(grid, marks, n_fields, where, among, cost, n_costs, cell=CELL):
    """cost_rule's fields for marks and costs in their layouts: ([env][field] (ny, nx) float32, (N, G) seed counts)."""
    marks, among, cost = _np(marks), None if among is None else _np(among), _np(cost)
    fields, counts = [], np.zeros((grid.n_envs, n_fields), np.int32)
    for e in range(grid.n_envs):
        geom, free, cells = _env(grid, e)
        row = []
        for g in range(n_fields):
            at = n_fields*cells.start + g*free.size
            seeds = seed_rule.seeds(free, marks[at:at + free.size].reshape(free.shape), where, None if among is None else among[cells].reshape(free.shape))
            counts[e, g] = seeds.sum()
            c = cost[cells] if n_costs == 1 else cost[at:at + free.size]
            row.append(cost_rule.field(free, cell, seeds, c.reshape(free.shape)))
        fields.append(row)
    return fields, counts


def _cost_of(fields, e, g):
    """(ny, nx) float32: the costs field (e, g) was made with."""
    first, ny, nx = fields.grid.cells(e)
    at = first if fields.n_costs == 1 else fields.n_goals*first + g*ny*nx
    return _np(fields.cost[at:at + ny*nx]).reshape(ny, nx)


def _fields_equal(grid, got, want):
    for e in range(grid.n_envs):
        for g in range(got.n_goals):
            have = _np(got.image(e, g))
            assert np.array_equal(bits(have), bits(want[e][g])), (e, g, int((bits(have) != bits(want[e][g])).sum()))


_THREE = {}


def _three():
    """Three small plans (two plain, one oblique), two agents each; two mark stores an env - a blob round an agent and a sprinkle of
    cells; the device's own clearance as an inflation layer (a store an env) and a random pricing of its own per field."""
    if not _THREE:
        from megastep_amd import cuda
        geoms = plans(2) + plans(1, oblique=True)
        c = _core(geoms, 2, 64)
        grid = cuda.nav_grid(c.scenery, clearance=RADIUS)
        rng = np.random.RandomState(21)
        marks = []
        for e in range(3):
            geom, free, _ = _env(grid, e)
            x, y = nav_rule.centres(geom, CELL)
            p = _np(c.agents.positions[e, 0])
            blob = (x[None, :] - p[0])**2 + (y[:, None] - p[1])**2 < 1.
            marks += [(blob.astype(np.uint8) | 2).reshape(-1), (rng.rand(*free.shape) < .01).astype(np.uint8).reshape(-1)]
        marks = torch.as_tensor(np.concatenate(marks), device='cuda')
        clear = cuda.clearance_fields(grid, c.scenery, max_range=1.)
        shared = cuda.inflation_costs(clear, .5)
        own = torch.as_tensor(np.exp(rng.uniform(-1, 4, 2*grid.n_cells)).astype(F), device='cuda')
        # (few cells may be a seed under where=False: were most of the floor seeds, most values would be 0 under any cost)
        among = torch.as_tensor((rng.rand(grid.free.shape[0]) < .003).astype(np.uint8), device='cuda')
        _THREE.update(core=c, geoms=geoms, grid=grid, marks=marks, clear=clear, shared=shared, own=own, among=among)
    return _THREE


@pytest.mark.parametrize('n_costs', [1, 2])
def test_cost_fields_are_the_rules_bits(n_costs):
    """Both variants; where=True without among and where=False among a layer; passes, n_seeds; the cost's builder is the formula."""
    from megastep_amd import cuda
    w = _three()
    grid, cost = w['grid'], w['shared'] if n_costs == 1 else w['own']
    assert np.array_equal(bits(_np(w['shared'])), bits(inflation(_np(w['clear'].values), .5)))
    for where, among in ((True, None), (False, w['among'])):
        want, counts = _rule_fields(grid, w['marks'], 2, where, among, cost, n_costs)
        flat, _ = _rule_fields(grid, w['marks'], 2, where, among, torch.ones_like(cost), n_costs)
        differ = total = 0
        for e in range(3):
            for g in range(2):
                both = np.isfinite(want[e][g])
                assert counts[e, g] > 0 and both.sum() > 500, (e, g)   # (an oblique plan's grid has free cells outside its walls)
                differ, total = differ + int((bits(want[e][g])[both] != bits(flat[e][g])[both]).sum()), total + int(both.sum())
        assert differ >= .25*total                                       # (a kernel that ignored the costs would fail)
        for which in (GLOBAL, IN_LDS, -1):
            with variant(which):
                got = cuda.cost_fields(grid, w['marks'], 2, cost, where=where, among=among, passes=True)
            assert isinstance(got, cuda.CostFields) and got.n_costs == n_costs and got.cost.data_ptr() == cost.data_ptr()
            assert got.n_seeds.dtype == torch.int32 and np.array_equal(_np(got.n_seeds), counts)
            _fields_equal(grid, got, want)
            assert (_np(got.passes) >= 2).all()
        print(f'n_costs={n_costs}, where={where}: seeds {counts.reshape(-1).tolist()}, passes {_np(got.passes).reshape(-1).tolist()}, '
              f'{differ} of {total} finite cells differ from the unweighted field')
    # a layer is a cost as it is
    layer = cuda.cost_fields(grid, w['marks'], 2, w['clear'] if n_costs == 1 else cuda.cell_layer(cost, 2))
    assert layer.n_costs == n_costs
    if n_costs == 2:
        assert torch.equal(layer.values.view(torch.int32), cuda.cost_fields(grid, w['marks'], 2, cost).values.view(torch.int32))


def test_a_mask_leaves_the_unmarked_fields_bits_alone():
    from megastep_amd import cuda
    w = _three()
    grid = w['grid']
    whole = cuda.cost_fields(grid, w['marks'], 2, w['own'], passes=True)
    mask = torch.tensor([[True, False], [False, False], [False, True]], device='cuda')
    some = cuda.cost_fields(grid, w['marks'], 2, w['own'], mask=mask)
    for e in range(3):
        for g in range(2):
            if mask[e, g]:
                assert torch.equal(some.image(e, g).view(torch.int32), whole.image(e, g).view(torch.int32))
            else:
                assert torch.isinf(some.image(e, g)).all() and int(some.n_seeds[e, g]) == 0
    kept_seeds = whole.n_seeds.clone()
    want = whole.values.clone()
    whole.values.fill_(SENTINEL); whole.passes.zero_(); whole.n_seeds.fill_(-3)
    for which in (GLOBAL, IN_LDS):
        with variant(which):
            assert cuda.cost_fields(grid, w['marks'], 2, w['own'], mask=mask, out=whole) is whole
        for e in range(3):
            for g in range(2):
                first, ny, nx = grid.cells(e)
                at = slice(2*first + g*ny*nx, 2*first + (g + 1)*ny*nx)
                if mask[e, g]:
                    assert torch.equal(whole.values[at].view(torch.int32), want[at].view(torch.int32))
                    assert int(whole.n_seeds[e, g]) == int(kept_seeds[e, g]) and int(whole.passes[e, g]) >= 2
                else:
                    assert (whole.values[at] == SENTINEL).all() and int(whole.n_seeds[e, g]) == -3 and int(whole.passes[e, g]) == 0


# ---------------------------------------------------------------------------------------------------------------------
# the tiers' edges
# ---------------------------------------------------------------------------------------------------------------------
def _capacities(which):
    from megastep_amd import _lib
    caps = (ctypes.c_int*3)()
    assert (_lib.lib().ms_host_nav_cost_capacity if which == IN_LDS else _lib.lib().ms_host_nav_field_capacity)(caps) == 0
    return tuple(caps)


def _framed_rectangle(framed, beyond):
    """(nx, ny) of an open rectangle whose frame holds exactly `framed` cells - or, `beyond`, the fewest cells above `framed` that
    make a rectangle at all (capacity + 1 where that has two factors of three or more)."""
    for total in ([framed] if not beyond else range(framed + 1, framed + 64)):
        pairs = [(a, total//a) for a in range(3, int(total**.5) + 1) if total % a == 0]
        if pairs:
            a, b = pairs[-1]                                            # (the squarest)
            return b - 2, a - 2
    raise AssertionError(framed)


_EDGES = {}


def _edge_world(nx, ny):
    """The boundary rectangle and an 8 x 8 one: open floor, a few seeds, and a gradient of costs with a ripple on it - so that the
    cheapest way is neither the straight one nor found in one pass."""
    if (nx, ny) not in _EDGES:
        rng = np.random.RandomState(nx*7 + ny)
        envs = [((-11, 4, nx, ny), np.ones((ny, nx), bool)), ((2, -3, 8, 8), np.ones((8, 8), bool))]
        marks, costs, want = [], [], []
        for _, free in envs:
            h, wd = free.shape
            m = (rng.rand(h, wd) < .002).astype(np.uint8)
            m[h//2, wd//2] = 1
            i, j = np.indices(free.shape)
            cost = (1 + 6*i/h + 3*j/wd + 2*np.sin(i*.9)*np.cos(j*.7) + rng.uniform(0, .5, free.shape)).astype(F)
            marks.append(m); costs.append(cost)
            want.append(cost_rule.field(free, CELL, m == 1, cost))
        assert len(np.unique(want[0])) > 1000 and np.isfinite(want[0]).all()
        _EDGES[nx, ny] = envs, marks, costs, want
    return _EDGES[nx, ny]


@pytest.mark.parametrize('beyond', [False, True], ids=['at', 'beyond'])
@pytest.mark.parametrize('tier', [0, 1, 2])
@pytest.mark.parametrize('which', [GLOBAL, IN_LDS], ids=['global', 'lds'])
def test_every_tier_of_either_variant_at_its_capacity_and_just_beyond(which, tier, beyond):
    """An open rectangle framed at exactly the variant's capacity for the tier, and at the capacity + 1 (the fewest cells more that
    frame a rectangle): the first relaxes in this tier's LDS, the second in the next one's - beyond the largest in global memory, in
    the same launch as an 8 x 8 env that stays in LDS."""
    from megastep_amd import cuda
    cap = _capacities(which)[tier]
    nx, ny = _framed_rectangle(cap, beyond)
    framed = (nx + 2)*(ny + 2)
    assert framed == cap if not beyond else cap < framed <= cap + 2, (cap, framed)
    envs, marks, costs, want = _edge_world(nx, ny)
    grid = _by_hand(envs)
    assert grid._max_framed == framed
    dev = lambda parts, pad: torch.as_tensor(np.concatenate([p.reshape(-1) for p in parts] + [pad]), device='cuda')
    m, c = dev(marks, np.zeros(0, np.uint8)), dev(costs, np.zeros(0, F))
    with variant(which):
        got = cuda.cost_fields(grid, m, 1, c, passes=True)
    for e in range(2):
        have = _np(got.image(e))
        assert np.array_equal(bits(have), bits(want[e])), (e, int((bits(have) != bits(want[e])).sum()))
    assert _np(got.n_seeds).reshape(-1).tolist() == [int(k.sum()) for k in marks] and (_np(got.passes) >= 2).all()
    print(f'{"LDS" if which else "global"} variant, tier {tier}, {nx} x {ny} = {framed} framed cells (capacity {cap}): passes '
          f'{_np(got.passes).reshape(-1).tolist()}')
    # the other variant, whatever tier it takes for this env, gives the same bits
    with variant(1 - which):
        other = cuda.cost_fields(grid, m, 1, c)
    assert torch.equal(other.values.view(torch.int32), got.values.view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------------
# the reduction and the clamp
# ---------------------------------------------------------------------------------------------------------------------
def test_a_cost_of_one_gives_seeded_fields_bits_on_the_device():
    from megastep_amd import cuda
    w = _three()
    grid = w['grid']
    rng = np.random.RandomState(2)
    low = rng.choice(np.array([0, -0., -3, -np.inf, 1e-40, -1e-45, .5, 1], F), 2*grid.n_cells)
    for where, among in ((True, None), (False, w['among'])):
        seeded = cuda.seeded_fields(grid, w['marks'], 2, where=where, among=among)
        assert torch.isfinite(seeded.values).sum() > 1000
        for cost in (torch.ones(grid.n_cells, device='cuda'), torch.ones(2*grid.n_cells, device='cuda'), torch.as_tensor(low, device='cuda')):
            for which in (GLOBAL, IN_LDS):
                with variant(which):
                    got = cuda.cost_fields(grid, w['marks'], 2, cost, where=where, among=among)
                assert torch.equal(got.values.view(torch.int32), seeded.values.view(torch.int32))
                assert torch.equal(got.n_seeds, seeded.n_seeds)


def test_costs_beyond_the_clamp_and_nans_count_as_256_on_the_device():
    from megastep_amd import cuda
    w = _three()
    grid = w['grid']
    odd, tame = clamp_layers((2*grid.n_cells,), np.random.RandomState(4))
    want, _ = _rule_fields(grid, w['marks'], 2, True, None, torch.as_tensor(tame), 2)
    for cost in (odd, tame):
        for which in (GLOBAL, IN_LDS):
            with variant(which):
                got = cuda.cost_fields(grid, w['marks'], 2, torch.as_tensor(cost, device='cuda'))
            _fields_equal(grid, got, want)
    nans = cuda.cost_fields(grid, w['marks'], 2, torch.full((grid.n_cells,), float('nan'), device='cuda'))
    dear = cuda.cost_fields(grid, w['marks'], 2, torch.full((grid.n_cells,), 256., device='cuda'))
    assert torch.equal(nans.values.view(torch.int32), dear.values.view(torch.int32))
    assert cuda.COST_MAX == 256.


# ---------------------------------------------------------------------------------------------------------------------
# the followers and the query
# ---------------------------------------------------------------------------------------------------------------------
def _follow_rule(grid, fields, points, which, lookahead=None, max_points=None, host=False, cell=CELL):
    """What cost_rule - or, `host`, the host instantiations - says for points (N, P, 2) following fields `which` (N, P)."""
    n, p = points.shape[:2]
    way, hops = np.full((n, p, 2), np.nan, F), np.full((n, p), -1, np.int32)
    paths, counts = np.full((n, p, max_points or 1, 2), np.nan, F), np.zeros((n, p), np.int32)
    for e in range(n):
        geom, free, _ = _env(grid, e)
        worlds = [(geom, cell, free, _np(fields.image(e, g))) for g in range(fields.n_goals)]
        costs = [_cost_of(fields, e, g) for g in range(fields.n_goals)]
        tables = [cost_rule.hops(world, cost) for world, cost in zip(worlds, costs)]
        for k in range(p):
            g = int(which[e, k])
            if not 0 <= g < fields.n_goals:
                continue
            if lookahead is not None:
                way[e, k], hops[e, k] = host_cost_follow(worlds[g], costs[g], points[e, k], lookahead=lookahead) if host else \
                    cost_rule.waypoint(worlds[g], points[e, k], lookahead, tables[g])
            if max_points is not None:
                paths[e, k], counts[e, k] = host_cost_follow(worlds[g], costs[g], points[e, k], max_points=max_points) if host else \
                    cost_rule.path(worlds[g], points[e, k], max_points, tables[g])
    return (way, hops) if max_points is None else (paths, counts)


@pytest.mark.parametrize('n_costs', [1, 2])
def test_cost_waypoints_paths_and_queries_are_the_rules_and_the_host_instantiations_bits(n_costs):
    from megastep_amd import cuda
    w = _three()
    grid = w['grid']
    fields = cuda.cost_fields(grid, w['marks'], 2, w['shared'] if n_costs == 1 else w['own'])
    rng = np.random.RandomState(17 + n_costs)
    points = _points(w['core'].scenery, w['geoms'], rng, spread=24, spawn=24)
    which = rng.randint(0, 2, points.shape[:2]).astype(np.int32)
    which[:, 5::11] = [[2, -1, 7, -3]]                               # no such field
    pts, goal = torch.as_tensor(points, device='cuda'), torch.as_tensor(which, device='cuda')
    # the query: the seeded one, on the weighted values
    have = _np(fields.at(pts, goal=goal))
    rule = np.full(which.shape, np.inf, F)
    for e in range(3):
        geom, free, _ = _env(grid, e)
        for k in range(which.shape[1]):
            if 0 <= which[e, k] < 2:
                rule[e, k] = seed_rule.query((geom, CELL, free, _np(fields.image(e, which[e, k]))), points[e, k])
    assert np.array_equal(bits(have), bits(rule)) and np.isfinite(rule).sum() > .3*rule.size
    seeded = cuda.SeededFields(grid, fields.marks, 2, True, None, fields.values, fields.n_seeds)
    assert torch.equal(seeded.at(pts, goal=goal).view(torch.int32), fields.at(pts, goal=goal).view(torch.int32))
    # the followers
    found = fields.paths(pts, goal=goal, max_points=24)
    want_paths, want_counts = _follow_rule(grid, fields, points, which, max_points=24)
    assert _equal(found.counts, want_counts) and _equal(found.points, want_paths)
    host_paths, host_counts = _follow_rule(grid, fields, points, which, max_points=24, host=True)
    assert _equal(found.counts, host_counts) and _equal(found.points, host_paths)
    ahead = 0
    for L in (1, 16, 64):
        way, hops = fields.waypoints(pts, goal=goal, lookahead=L, hops=True)
        want_way, want_hops = _follow_rule(grid, fields, points, which, lookahead=L)
        assert _equal(hops, want_hops) and _equal(way, want_way), L
        host_way, host_hops = _follow_rule(grid, fields, points, which, lookahead=L, host=True)
        assert _equal(hops, host_hops) and _equal(way, host_way), L
        assert torch.equal(hops < 0, torch.isinf(fields.at(pts, goal=goal))) and torch.equal(torch.isnan(way).any(-1), hops < 0)
        ahead += (want_hops >= 2).sum()
    assert ahead > 20 and (want_counts >= 0).all() and (want_counts > 24).any() and (want_counts == 0).any()
    # the weighted hop is not the unweighted one: the seeded followers on the same values go another way somewhere
    plain = seeded.paths(pts, goal=goal, max_points=24)
    assert not torch.equal(plain.points.view(torch.int32), found.points.view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------------
# costs rewritten in place
# ---------------------------------------------------------------------------------------------------------------------
def test_update_and_a_captured_graph_follow_costs_rewritten_in_place():
    from megastep_amd import cuda
    w = _three()
    grid = w['grid']
    cost = w['own'].clone()
    fields = cuda.cost_fields(grid, w['marks'], 2, cost)
    before = fields.values.clone()
    rng = np.random.RandomState(8)
    pts = torch.as_tensor(_points(w['core'].scenery, w['geoms'], rng, spread=0, spawn=2), device='cuda')
    layers = [torch.as_tensor(np.exp(rng.uniform(-1, 5, cost.shape[0])).astype(F), device='cuda') for _ in range(3)]
    cost.copy_(layers[0])
    assert fields.update() is fields and not torch.equal(fields.values.view(torch.int32), before.view(torch.int32))
    assert torch.equal(fields.values.view(torch.int32), cuda.cost_fields(grid, w['marks'], 2, layers[0]).values.view(torch.int32))
    # a builder rewriting its layer in place, then update(): known-space costs over marks that change
    seen = torch.zeros_like(w['marks'])
    known = cuda.mark_costs(cuda.cell_layer(seen, 2))
    routes = cuda.cost_fields(grid, w['marks'], 2, known)
    assert (known == 256).all() and (routes.values[torch.isfinite(routes.values)] >= 0).all()
    seen.fill_(1)
    assert cuda.mark_costs(cuda.cell_layer(seen, 2), out=known) is known and (known == 1).all()
    routes.update()
    assert torch.equal(routes.values.view(torch.int32), cuda.seeded_fields(grid, w['marks'], 2).values.view(torch.int32))
    # captured once, replayed on costs changed in place
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fields.update(); fields.waypoints(pts, hops=True)
    torch.cuda.current_stream().wait_stream(side)
    with torch.cuda.graph(graph):
        fields.update()
        way, hops = fields.waypoints(pts, hops=True)
    for layer in layers[1:]:
        cost.copy_(layer)
        graph.replay()
        eager = cuda.cost_fields(grid, w['marks'], 2, layer)
        assert torch.equal(fields.values.view(torch.int32), eager.values.view(torch.int32))
        want_way, want_hops = eager.waypoints(pts, hops=True)
        assert torch.equal(way.view(torch.int32), want_way.view(torch.int32)) and torch.equal(hops, want_hops) and (hops >= 0).any()


# ---------------------------------------------------------------------------------------------------------------------
# modules and the env
# ---------------------------------------------------------------------------------------------------------------------
def test_routes_under_the_path_follower_and_frontiers_with_a_cost():
    from megastep_amd import cuda, modules
    w = _three()
    c, grid, geoms = w['core'], w['grid'], w['geoms']
    goals = modules.Goals(geoms, c, grid)
    everyone = c.agent_full(True)
    goals(everyone)
    routes = modules.Routes(c, grid, goals, w['shared'])
    fields = routes(everyone)
    assert isinstance(fields, cuda.CostFields) and fields is routes.fields and fields.n_goals == 2
    by_hand = cuda.cost_fields(grid, cuda.point_marks(grid, goals.goals, 2).marks, 2, w['shared'])
    assert torch.equal(fields.values.view(torch.int32), by_hand.values.view(torch.int32)) and (fields.n_seeds > 0).any()
    way, d = routes.waypoints(16), routes.distances()
    assert way.shape == (3, 2, 2) and d.shape == (3, 2) and torch.equal(torch.isnan(way).any(-1), torch.isinf(d))
    assert torch.equal(way.view(torch.int32), by_hand.waypoints(c.agents.positions).view(torch.int32))
    assert torch.equal(torch.isinf(d), torch.isinf(goals.distances())) and (d[torch.isfinite(d)] >= goals.distances()[torch.isfinite(d)] - 2*CELL).all()
    follower = modules.PathFollower(c, routes)
    actions = follower().actions
    assert actions.shape == (3, 2) and actions.dtype == torch.int64 and ((actions >= 0) & (actions < 7)).all()
    # new goals for some: only their routes change
    held = fields.values.clone()
    some = torch.tensor([[True, False], [False, False], [False, True]], device='cuda')
    goals(some)
    routes(some)
    by_hand = cuda.cost_fields(grid, cuda.point_marks(grid, goals.goals, 2).marks, 2, w['shared'])
    assert torch.equal(fields.values.view(torch.int32), by_hand.values.view(torch.int32))
    first, ny, nx = grid.cells(1)
    assert torch.equal(fields.values[2*first:2*first + 2*ny*nx].view(torch.int32), held[2*first:2*first + 2*ny*nx].view(torch.int32))
    # frontiers over a known-space layer
    for shared in (False, True):
        cover = modules.Coverage(c, grid, max_range=4., shared=shared)
        cover(modules.render(c, fields=('distances',)))
        known = cuda.mark_costs(cover.maps)
        frontiers = modules.Frontiers(c, cover, refresh=4, cost=known)
        assert isinstance(frontiers.fields, cuda.CostFields) and frontiers.fields.n_costs == frontiers.fields.n_goals == (1 if shared else 2)
        frontiers()
        by_hand = cuda.cost_fields(grid, cover.maps.values, cover.maps.n_maps, known, where=False, among=cover.maps.countable)
        assert torch.equal(frontiers.fields.values.view(torch.int32), by_hand.values.view(torch.int32))
        way, d = frontiers.waypoints(), frontiers.distance()
        assert way.shape == (3, 2, 2) and torch.equal(torch.isnan(way).any(-1), torch.isinf(d)) and torch.isfinite(d).any()
        plain = modules.Frontiers(c, cover, refresh=4)
        assert type(plain.fields) is cuda.SeededFields and (d >= plain.distance()).all()


def _captured(step):
    """`step` warmed up once on a side stream, then captured: (graph, what the captured call returned)."""
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    return graph, out


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32)) if a.dtype == torch.float32 else torch.equal(a, b)


@pytest.mark.parametrize('kind', ['own maps', 'shared map', 'territories'])
def test_frontiers_with_a_cost_replayed_from_a_graph_equal_the_eager_module(kind):
    """Two Frontiers over one Coverage and one known-space layer, refresh 2: one called eagerly, one captured after its first call
    and replayed. Before every step the agents turn and are seen further, one agent starts over, and the layer is rewritten in place
    by mark_costs(out=) - inside the captured step too. Fields, due masks, distances and waypoints are equal bit for bit at every
    step; the fields that were due at a step are cost_fields called by hand."""
    from megastep_amd import cuda, modules
    w = _three()
    c, grid = w['core'], w['grid']
    shared = kind != 'own maps'
    cover = modules.Coverage(c, grid, max_range=4., shared=shared)
    cover(modules.render(c, fields=('distances',)))
    known = [cuda.mark_costs(cover.maps) for _ in range(2)]
    reset = torch.zeros((3, 2), dtype=torch.bool, device='cuda')
    pair = [modules.Frontiers(c, cover, refresh=2, cost=known[k], territories=modules.Territories(c, grid, refresh=2) if kind == 'territories' else None)
            for k in range(2)]
    assert all(isinstance(f.fields, cuda.CostFields) for f in pair) and (kind != 'territories' or all(isinstance(f.own, cuda.CostFields) for f in pair))

    def step(k):
        cuda.mark_costs(cover.maps, out=known[k])
        pair[k](reset)
        return pair[k].distance(), pair[k].waypoints()

    step(0)                                                             # (the first call of each: everything is due)
    graph, (d, way) = _captured(lambda: step(1))                        # (the warm-up is the graphed module's first call)
    angles, positions = c.agents.angles.clone(), c.agents.positions.clone()
    moved = False
    try:
        for t in range(4):
            c.agents.angles[:] = angles + 70.*(t + 1)
            cover(modules.render(c, fields=('distances',)))
            if t == 2:
                c.agents.positions[:, 0] = positions[:, 1]                # (agent 0 starts over where agent 1 stands)
            reset.zero_()
            reset[t % 3, t % 2] = t != 1
            want_d, want_way = step(0)
            graph.replay()
            eager, graphed = pair
            assert _same_bits(graphed.fields.values, eager.fields.values) and torch.equal(graphed.fields.n_seeds, eager.fields.n_seeds), t
            assert _same_bits(known[1], known[0]) and _same_bits(d, want_d) and _same_bits(way, want_way), t
            assert torch.isfinite(d).any() and torch.equal(torch.isnan(way).any(-1), torch.isinf(d))
            if kind == 'territories':
                assert _same_bits(graphed.own.values, eager.own.values) and torch.equal(graphed.own.n_seeds, eager.own.n_seeds), t
            # the fields that were due at this step - an agent's every second step, and at once when it starts over; with a shared
            # map an env's one field when any of its agents is - are cost_fields called by hand
            maps = cover.maps
            due = graphed.due.any(-1, keepdim=True) if shared else graphed.due
            assert torch.equal(graphed.due, eager.due) and due.any() and (t % 2 == 0 or due.sum() >= due.numel() - 2)
            by_hand = cuda.cost_fields(grid, maps.values, maps.n_maps, cuda.mark_costs(maps), where=False, among=maps.countable)
            own = cuda.cost_fields(grid, graphed.territories.masks.values, 2, cuda.mark_costs(maps), where=True, among=graphed._unseen) \
                if kind == 'territories' else None
            for e in range(3):
                first, ny, nx = grid.cells(e)
                G = maps.n_maps
                for g in range(G):
                    at = slice(G*first + g*ny*nx, G*first + (g + 1)*ny*nx)
                    if due[e, g]:
                        assert _same_bits(graphed.fields.values[at], by_hand.values[at]), (t, e, g)
                if own is not None and due[e, 0]:
                    assert _same_bits(graphed.own.values[2*first:2*first + 2*ny*nx], own.values[2*first:2*first + 2*ny*nx]), (t, e)
            moved = moved or not _same_bits(known[1], torch.full_like(known[1], 256.))
        assert moved
    finally:
        c.agents.angles[:] = angles
        c.agents.positions[:] = positions


def test_routes_under_the_path_follower_replayed_from_a_graph_equal_the_eager_modules():
    """Goals -> inflation_costs(out=) -> Routes -> PathFollower as one captured step, next to an eager twin over the same table: the
    clearance is rewritten in place, agents are moved and some start over between the steps; costs, fields, waypoints and actions
    are equal bit for bit, and the fields are cost_fields called by hand."""
    from megastep_amd import cuda, modules
    w = _three()
    c, grid, geoms = w['core'], w['grid'], w['geoms']
    table = torch.as_tensor(modules.random_empty_positions(geoms, 2, 12), dtype=torch.float32, device='cuda')
    clear = cuda.clearance_fields(grid, c.scenery, max_range=1.)
    reset = c.agent_full(True)
    twins = []
    for k in range(2):
        goals = modules.Goals(geoms, c, grid, table=table)
        cost = cuda.inflation_costs(clear, .5)
        routes = modules.Routes(c, grid, goals, cost)
        twins.append((goals, cost, routes, modules.PathFollower(c, routes)))

    def step(k):
        goals, cost, routes, follower = twins[k]
        cuda.inflation_costs(clear, .5, out=cost)
        goals(reset)
        routes(reset)
        return follower().actions, routes.waypoints(16)

    step(0)
    graph, (actions, way) = _captured(lambda: step(1))
    positions, held = c.agents.positions.clone(), clear.values.clone()
    try:
        for t in range(3):
            c.agents.positions[:] = table[:, :, 3 + t]
            clear.values.mul_(.8)                                       # (the walls "come nearer": every cost within reach rises)
            reset.zero_()
            reset[t, t % 2] = True
            want_actions, want_way = step(0)
            graph.replay()
            (_, cost0, eager, _), (goals, cost1, graphed, _) = twins
            assert _same_bits(cost1, cost0) and np.array_equal(bits(_np(cost1)), bits(inflation(_np(clear.values), .5))), t
            assert _same_bits(graphed.fields.values, eager.fields.values) and _same_bits(way, want_way) and torch.equal(actions, want_actions), t
            assert ((actions >= 0) & (actions < 7)).all() and torch.isfinite(way).any()
        # every field again from the costs as they stand: cost_fields by hand
        reset.fill_(True)
        step(0); graph.replay()
        by_hand = cuda.cost_fields(grid, cuda.point_marks(grid, goals.goals, 2).marks, 2, cost1)
        assert _same_bits(graphed.fields.values, by_hand.values) and _same_bits(graphed.fields.values, eager.fields.values)
    finally:
        c.agents.positions[:] = positions
        clear.values.copy_(held)


class _Expert:
    """An env whose step is the expert's: the decision handed in is ignored."""

    def __init__(self, env):
        self.env = env

    def __getattr__(self, name):
        return getattr(self.env, name)

    def step(self, decision):
        return self.env.step(self.env.expert())


def test_pointgoal_with_a_margin_steps_eager_and_as_one_graph():
    from megastep_amd import arrdict, cuda, graphs
    from megastep_amd.demo.envs.pointgoal import PointGoal
    logs = []
    for graphed in (False, True):
        torch.manual_seed(3); np.random.seed(3)
        env = PointGoal(8, geometries=plans(8), margin=.3)
        assert isinstance(env._follower.goals, type(env._routes)) and env.costs.shape == env.clearance.values.shape
        stepper = graphs.GraphedStep(_Expert(env), warmup=3) if graphed else _Expert(env)
        stepper.reset()
        nothing = arrdict.arrdict(actions=torch.zeros((8, 1), dtype=torch.long, device='cuda'))
        log = []
        for t in range(10 if graphed else 13):
            world = stepper.step(nothing)
            log.append((world.reward.clone(), world.reset.clone(), env.core.agents.positions.clone(), env._routes.fields.values.clone()))
        logs.append(log)
        by_hand = cuda.cost_fields(env.grid, cuda.point_marks(env.grid, env._goals.goals, 1).marks, 1, env.costs)
        assert torch.equal(env._routes.fields.values.view(torch.int32), by_hand.values.view(torch.int32))
        assert np.array_equal(bits(_np(env.costs)), bits(inflation(_np(env.clearance.values), .3)))
    eager, graphed = logs
    for k in range(10):
        for got, want in zip(graphed[k], eager[k + 3]):
            assert torch.equal(got, want), k
    assert not torch.equal(graphed[0][2], graphed[-1][2])                # (they moved)
    # without a margin nothing is built and the follower is the goals' own
    plain = PointGoal(8, geometries=plans(8))
    assert plain._routes is None and plain.costs is None and plain._follower.goals is plain._goals
