"""View fields on the GPU (cuda.view_fields, ViewFields.update, modules.BestViews, FloorCoverage.expert('views')): the kernel is
held to EQUALITY with tests/test_navview_host.py's view_rule - bytes, counts and gains - on the six plans, on a large plan whose
kept walls overflow the LDS, and on the hand-made worlds; then what is built on it."""
import numpy as np
import pytest
import torch

from tests.test_navfield_host import CELL, RADIUS, F, plans, spawn_points
from tests.test_navview_host import CONE, box_walls, hand, plan_views, same, view_rule
from tests.test_gpu_navseen import _np, _six

pytestmark = pytest.mark.gpu


def _walls(scenery):
    """[(L, 4) float32] per env: the scenery's static rows, read back."""
    lines = scenery.lines
    af = scenery.n_agents*scenery.model.shape[0]
    vals, starts, widths = _np(lines.vals).reshape(-1, 4), _np(lines.starts), _np(lines.widths)
    return [vals[starts[e] + af:starts[e] + widths[e]] for e in range(len(widths))]


def _result(v):
    return dict(values=_np(v.values), counts=_np(v.counts), gains=_np(v.gains))


def _rule(v, walls, mask=None, before=None, images=None):
    """view_rule on a mirror of what the ViewFields ``v`` reads, as it stands."""
    grid, maps = v.grid, v.unseen
    cone = v.headings is not None
    return view_rule.call(grid._host_geom, grid._host_starts, grid.cell, walls, _np(v.points), v.max_range, _np(v.countable),
                          headings=_np(v.headings), cos_half=v.cos_half if cone else None, unseen=None if maps is None else _np(maps.values),
                          S=0 if maps is None else maps.n_maps, slot=_np(v.slot), mask=_np(mask), before=before, images=images)


def _same(v, walls, mask=None, before=None, images=None):
    want = _rule(v, walls, mask, before, images)
    same(_result(v), want, tuple(k for k in ('values', 'counts', 'gains') if getattr(v, k) is not None))
    return want


_WORLD = {}


def _world():
    """The six plans' grid, seen maps marked by one rendered frame, the host suite's viewpoints and the walls read back."""
    if not _WORLD:
        from megastep_amd import cuda
        c = _six()['core']
        grid = cuda.nav_grid(c.scenery, clearance=RADIUS)
        maps = cuda.seen_maps(grid, 2)
        maps.mark(*_six()['frames'][0])
        w = plan_views()
        walls = _walls(c.scenery)
        assert all(np.array_equal(a, b) for a, b in zip(walls, w.walls)) and np.array_equal(grid._host_geom, w.geom)
        _WORLD.update(core=c, grid=grid, maps=maps, walls=walls, host=w, points=torch.as_tensor(w.points, device='cuda'),
                      headings=torch.as_tensor(w.headings, device='cuda'))
    return _WORLD


@pytest.mark.parametrize('cone', [False, True])
@pytest.mark.parametrize('R', [4., 10.])
def test_view_fields_are_the_rules_on_the_six_plans(R, cone):
    from megastep_amd import cuda
    w = _world()
    kw = dict(headings=w['headings'], fov=CONE) if cone else {}
    v = cuda.view_fields(w['grid'], w['core'].scenery, w['points'], R, unseen=w['maps'], **kw)
    assert isinstance(v, cuda.ViewFields) and v.n_points == 2 and v.values.dtype == torch.uint8 and v.counts.dtype == v.gains.dtype == torch.int32
    assert v.counts.shape == v.gains.shape == (6, 2) and v.countable is w['maps'].countable
    want = _same(v, w['walls'], images=w['host'].vis[R, cone])           # (the rule's images: the CPU suite's, of the same walls and points)
    assert (want['counts'] > 0).all() and 0 < want['gains'].sum() < want['counts'].sum()
    first, ny, nx = w['grid'].cells(3)
    assert v.image(3, 1).shape == (ny, nx) and v.image(3, 1).dtype == torch.bool
    assert torch.equal(v.image(3, 1).reshape(-1), v.values[2*first + ny*nx:2*first + 2*ny*nx].bool())
    bare = cuda.view_fields(w['grid'], w['core'].scenery, w['points'], R, unseen=w['maps'], store=False, **kw)
    assert bare.values is None and torch.equal(bare.counts, v.counts) and torch.equal(bare.gains, v.gains)
    # one map an env; a slot; a countable mask of one's own and no maps at all
    one = cuda.seen_maps(w['grid'], 1)
    one.values.copy_(w['maps'].values[:one.values.shape[0]])
    _same(cuda.view_fields(w['grid'], w['core'].scenery, w['points'], R, unseen=one, store=False, **kw), w['walls'], images=w['host'].vis[R, cone])
    slot = torch.tensor([[1, 0], [0, 0], [1, 1], [2, 0], [0, -1], [1, 0]], device='cuda')
    got = cuda.view_fields(w['grid'], w['core'].scenery, w['points'], R, unseen=w['maps'], slot=slot, store=False, **kw)
    _same(got, w['walls'], images=w['host'].vis[R, cone])
    assert got.gains[3, 0] == 0 and got.gains[4, 1] == 0
    countable = torch.as_tensor(np.random.RandomState(3).rand(w['grid'].free.shape[0]) < .6, device='cuda')
    plain = cuda.view_fields(w['grid'], w['core'].scenery, w['points'], R, countable=countable, **kw)
    assert plain.gains is None
    _same(plain, w['walls'], images=w['host'].vis[R, cone])


def test_a_large_plan_whose_kept_walls_overflow_the_lds():
    from megastep_amd import cuda, scene
    geoms = plans(1, large=True)
    walls = np.asarray(geoms[0]['walls'], F).reshape(-1, 4)
    R = 10.
    lo, hi = np.minimum(walls[:, :2], walls[:, 2:]), np.maximum(walls[:, :2], walls[:, 2:])
    sp = spawn_points(geoms[0])
    kept = np.array([((lo <= p + F(R)) & (hi >= p - F(R))).all(1).sum() for p in sp])     # (a box inside the kernel's: at least these are kept)
    points = np.stack([sp[kept.argmax()], sp[kept.argmin()]])[None].astype(F)
    assert kept.max() > cuda.VIEW_WALL_CAPACITY >= kept.min()
    sc = scene.scenery(geoms, 1, device='cuda', bake=False)
    grid = cuda.nav_grid(sc, clearance=RADIUS)
    v = cuda.view_fields(grid, sc, torch.as_tensor(points, device='cuda'), R)
    want = _same(v, _walls(sc))
    assert (want['counts'] > 200).all()
    print('kept walls:', int(kept.max()), int(kept.min()), 'of', len(walls), '- visible free cells:', want['counts'].reshape(-1).tolist())


def _hand_world():
    """tests/test_navview_host.hand() on the device: its walls as a scenery of two agents an env (the NaN row put in afterwards),
    its grid laid out by hand - env 2 without cells, envs 2 and 3 without static walls."""
    from megastep_amd import cuda, scene
    w = hand()
    geoms = []
    for n in range(5):
        walls = w.walls[n].copy()
        if n == 0:
            walls[3] = (1, 1, 3, 3)
        geoms.append(dict(walls=walls.reshape(-1, 2, 2), lights=np.array([[1., 1.]])))
    sc = scene.scenery(geoms, 2, device='cuda', bake=False)
    af = 2*sc.model.shape[0]
    sc.lines.vals[int(sc.lines.starts[0]) + af + 3] = torch.tensor([[float('nan'), 1.], [3., float('nan')]], device='cuda')
    got = _walls(sc)
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(got, w.walls)) and np.isnan(got[0][3]).any()
    dev = lambda a: torch.as_tensor(a, device='cuda')
    free = np.concatenate([w.free, np.zeros(1, np.uint8)])
    grid = cuda.NavGrid(dev(w.geom), dev(w.starts), dev(free), CELL, RADIUS, w.geom, w.starts)
    maps = cuda.seen_maps(grid, 8)
    maps.values.copy_(dev(w.seen))
    return w, sc, grid, maps


def test_the_odd_cases_in_one_ragged_call():
    from megastep_amd import cuda
    w, sc, grid, maps = _hand_world()
    points, headings = torch.as_tensor(w.points, device='cuda'), torch.as_tensor(w.headings, device='cuda')
    for R, cone in ((20., False), (2., True), (.75, False), (.05, False)):
        kw = dict(headings=headings, fov=CONE) if cone else {}
        v = cuda.view_fields(grid, sc, points, R, unseen=maps, **kw)
        want = _same(v, w.walls)
        assert (want['counts'][2] == 0).all() and (want['gains'][2] == 0).all()          # (the env without cells)
        if R == 20.:
            assert not v.image(0, 4).any() and v.counts[0, 4] == 0 and v.image(0, 1).sum() > 1000 and v.image(3, 0).all()
        if cone:
            assert v.counts[0, 0] == 0 and v.counts[3, 2] == 0 and v.counts[4, 1] == 0    # (headings without a length)
        if R == .05:
            assert v.image(0, 2).sum() == 1 and v.image(3, 1).sum() == 1


def test_mask_out_update_a_side_stream_and_a_graph_replayed_three_times():
    from megastep_amd import cuda
    w = _world()
    grid, sc, walls = w['grid'], w['core'].scenery, w['walls']
    frames = _six()['frames']
    maps = cuda.seen_maps(grid, 2)
    points, R = w['points'].clone(), 4.
    # a fresh call with a mask: the other viewpoints see nothing
    mask = torch.as_tensor(np.random.RandomState(6).rand(6, 2) < .5, device='cuda')
    mask[0, 0], mask[0, 1] = True, False
    v = cuda.view_fields(grid, sc, points, R, unseen=maps, mask=mask)
    first = _same(v, walls, mask)
    assert first['counts'][0, 1] == 0 and first['counts'][0, 0] > 0 and np.array_equal(first['gains'], first['counts'])
    # update(mask) in place after the points moved and a frame was marked: the masked-out viewpoints keep what they held
    tensors = (v.values, v.counts, v.gains)
    points += torch.tensor([.1, -.05], device='cuda')
    maps.mark(*frames[0])
    assert v.update(~mask) is v
    second = _same(v, walls, ~mask, first)
    assert not np.array_equal(second['values'], first['values']) and (second['gains'] <= second['counts']).all()
    # out=: the same tensors, this call's arguments
    maps.mark(*frames[1])
    got = cuda.view_fields(grid, sc, points, 5., unseen=maps, mask=mask, out=v)
    assert got is v and v.max_range == 5. and all(x is y for x, y in zip(tensors, (v.values, v.counts, v.gains)))
    _same(v, walls, mask, second)
    for kw in (dict(store=False), dict(unseen=None), dict(points=points[:, :1].contiguous(), slot=torch.zeros((6, 1), dtype=torch.int32, device='cuda'))):
        with pytest.raises(RuntimeError, match='`out` must come from a view_fields call'):
            cuda.view_fields(grid, sc, **{**dict(points=points, unseen=maps), **kw}, out=v)
    # a side stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        v.update()
    side.synchronize()
    _same(v, walls)
    # captured once, replayed three times, the points moved and the maps marked in between
    maps.values.zero_()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        v.update()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        v.update()
    gains = []
    for replay in range(3):
        if replay:
            maps.mark(*frames[replay - 1])
            points += torch.tensor([-.06, .04], device='cuda')
        graph.replay()
        gains.append(_same(v, walls)['gains'].copy())
    assert (gains[0] > 0).all() and gains[1].sum() < gains[0].sum() and not np.array_equal(gains[1], gains[2])


def test_the_views_are_a_layer_for_seeded_fields_cell_draws_and_local_maps():
    from megastep_amd import cuda
    from tests.test_gpu_navseed import _fields_equal, _rule_fields
    from tests.test_gpu_navwindow import _same as same_window
    w = _world()
    grid = w['grid']
    v = cuda.view_fields(grid, w['core'].scenery, w['points'], 4.)
    # the walking distance to cover: to the nearest free cell the viewpoint does not see
    cover = cuda.seeded_fields(grid, v.values, 2, where=False)
    want, counts = _rule_fields(grid, v.values, 2, False, None)
    assert _fields_equal(grid, cover, want) == 12 and np.array_equal(_np(cover.n_seeds), counts)
    at = cover.at(w['points'])
    assert torch.isfinite(at).all() and (at > 0).all()                   # (a viewpoint sees the cells round it: cover is a walk away)
    # hiding spots: draws among the free cells out of sight
    draws = cuda.cell_draws(grid, v, 2, 64, where=False, seed=9)
    starts = torch.as_tensor(grid._host_starts[:-1], device='cuda')[:, None, None]
    sizes = torch.as_tensor((grid._host_starts[1:] - grid._host_starts[:-1]), device='cuda')[:, None, None]
    store = 2*starts + torch.arange(2, device='cuda')[None, :, None]*sizes + draws.cells
    assert (draws.cells >= 0).all() and (v.values[store.reshape(-1)] == 0).all() and (grid.free[(starts + draws.cells).reshape(-1)] == 1).all()
    hidden = torch.stack([torch.stack([(grid.image(e) & ~v.image(e, p)).sum() for p in range(2)]) for e in range(6)])
    assert torch.equal(draws.counts.long(), hidden)
    # a channel of the views
    views = cuda.agent_views(w['core'].agents, 16, 3.)
    got = _np(same_window(grid, views, 16, [cuda.map_channel(v), cuda.map_channel(v, where=False, gate=grid)]))
    assert (got[:, :, 0] == 1).any() and (got[:, :, 0] == 0).any() and (got[:, :, 1] == 1).any()
    assert cuda.cell_layer(v).values is v.values and cuda.cell_layer(v).n_fields == 2


def _restated_choice(gains, distances, d0=1.):
    """BestViews.choose by another road: the leading candidates that fall short of the best score are counted."""
    valid = torch.isfinite(distances) & (gains > 0)
    score = torch.where(valid, gains.float()/(distances + d0), torch.full_like(distances, -1.))
    index = (score == score.amax(-1, keepdim=True)).int().cumsum(-1).eq(0).sum(-1)
    return index, ~valid.any(-1)


def _goals_are_the_choice(env):
    from megastep_amd import cuda
    bv = env._views
    here = env.core.agents.positions
    index, none = _restated_choice(bv.gains, bv.distances)
    picked = bv.candidates.gather(2, index[..., None, None].expand(-1, -1, 1, 2)).squeeze(2)
    assert torch.equal(bv.none, none) and torch.equal(bv.goals, torch.where(none[..., None], here, picked)) and (~none).any()
    # the gains are view_fields' of the candidates against the maps as they stand; every goal can be walked to
    n, a, k = bv.gains.shape
    slot = torch.arange(a, device='cuda')[None, :, None].expand(n, a, k).reshape(n, a*k)
    fresh = cuda.view_fields(env.grid, env.core.scenery, bv.candidates.reshape(n, a*k, 2).clone(), bv.max_range, unseen=env.maps, slot=slot, store=False)
    assert torch.equal(fresh.gains.reshape(n, a, k), bv.gains) and (bv.gains > 0).any()
    assert torch.isfinite(cuda.geodesic(env.grid, here.contiguous(), bv.goals.contiguous())).all()


def test_best_views_goals_are_the_choice_among_their_own_candidates():
    from megastep_amd import modules
    from megastep_amd.demo import FloorCoverage
    torch.manual_seed(5); np.random.seed(5)
    env = FloorCoverage(8, n_agents=2, geometries=plans(8), max_lifespan=10**6)
    env.reset()
    decision = env.expert('views')                                        # (everyone started over: everyone is due)
    bv = env._views
    assert isinstance(bv, modules.BestViews) and bv.candidates.shape == (8, 2, 16, 2) and bv.gains.shape == bv.distances.shape == (8, 2, 16)
    assert bool(bv.frontiers.due.all())
    _goals_are_the_choice(env)
    held = bv.goals.clone()
    for _ in range(8):                                                   # (eight steps on everyone is due again)
        env.step(decision)
        decision = env.expert('views')
    assert bool(bv.frontiers.due.all())
    _goals_are_the_choice(env)
    assert not torch.equal(held, bv.goals)
    waypoints = bv.waypoints()
    assert waypoints.shape == (8, 2, 2) and torch.isfinite(waypoints[~bv.none]).all()


def _rollout(env, steps, policy, seed=1):
    """`steps` steps under env.expert(policy) or uniformly random actions: (episodes ended by coverage, by lifespan, the mean over
    all episodes - those still running at the end included - of the fraction seen at their last step)."""
    from megastep_amd import arrdict
    rng = np.random.RandomState(seed)
    n, a = env.core.n_envs, env.core.n_agents
    env.reset()
    by_coverage = by_lifespan = 0
    final = []
    for t in range(steps):
        fraction = env._coverage.fraction().clone()
        over = env._over.clone()
        done = fraction >= env.complete
        by_coverage += int((over & done).sum())
        by_lifespan += int((over & ~done).sum())
        final += fraction[over].tolist()
        decision = arrdict.arrdict(actions=torch.as_tensor(rng.randint(0, 7, (n, a)), device='cuda')) if policy == 'random' else env.expert(policy)
        env.step(decision)
    final += env._coverage.fraction().reshape(-1).tolist()
    return by_coverage, by_lifespan, float(np.mean(final))


def test_the_views_expert_sees_the_floor_at_least_as_well_as_a_random_policy():
    """FloorCoverage(32), 200 steps, under expert('views'), expert('frontier') and uniformly random actions, the same seeds: the
    views expert's mean final fraction is not below the random policy's (the frontier test's condition); all three are printed."""
    from megastep_amd.demo import FloorCoverage
    results = {}
    for policy in ('views', 'frontier', 'random'):
        torch.manual_seed(3); np.random.seed(3)
        env = FloorCoverage(32, geometries=plans(32), max_lifespan=200)
        results[policy] = _rollout(env, 200, policy)
        print(f'FloorCoverage(32), 200 steps, {policy}: {results[policy][0]} episodes ended by coverage, {results[policy][1]} by lifespan, '
              f'mean final fraction {results[policy][2]:.3f}')
    assert results['views'][2] >= results['random'][2], results


class _Expert:
    """An env whose step is the views expert's: the decision handed in is ignored."""

    def __init__(self, env):
        self.env = env

    def __getattr__(self, name):
        return getattr(self.env, name)

    def step(self, decision):
        return self.env.step(self.env.expert('views'))


def test_the_views_expert_and_the_step_as_one_hip_graph_equal_the_eager_env():
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
            log.append((world.reward.clone(), world.reset.clone(), env.maps.values.clone(), env.core.agents.positions.clone(), env._views.goals.clone()))
        logs.append(log)
    eager, graphed = logs
    for k in range(10):
        for got, want in zip(graphed[k], eager[k + 3]):
            assert torch.equal(got, want), k
    assert sum(float(r.sum()) for r, _, _, _, _ in graphed) > 0
    assert not torch.equal(graphed[0][3], graphed[-1][3])                # (they moved)
