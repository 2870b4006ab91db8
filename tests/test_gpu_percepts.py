"""Percepts on the GPU (cuda.percepts, modules.Percepts, demo.Tag): the kernel is held to EQUALITY with tests/percept_rule.py in
every output - on the six plans with the CPU suite's eyes and points, on a large plan whose kept walls overflow the LDS, on the
hand-made shapes round a wave's 64 points and a workgroup's four eyes - and pinned to the view fields' bytes; then what is built
on it."""
import numpy as np
import pytest
import torch

from tests.percept_rule import KEYS, hand_shape, percept_rule, plan_percepts, plan_rule, same
from tests.test_navfield_host import RADIUS, F, plans, spawn_points
from tests.test_navview_host import CONE, plan_views
from tests.test_gpu_navseen import _np, _six
from tests.test_gpu_navview import _walls

pytestmark = pytest.mark.gpu


def _dev(a, dtype=None):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), device='cuda', dtype=dtype)


def _result(seen):
    return {k: _np(getattr(seen, k)) for k in KEYS if getattr(seen, k) is not None}


def _call(scenery, w, R, K, cone=False, valid=None, pairs=None, mask=None, **kw):
    from megastep_amd import cuda
    if cone:
        kw.update(headings=_dev(w.headings), fov=CONE)
    return cuda.percepts(scenery, _dev(w.points), eyes=_dev(w.eyes), max_range=R, k=K, valid=_dev(valid), pairs=_dev(pairs), mask=_dev(mask), **kw)


@pytest.mark.parametrize('cone', [False, True])
@pytest.mark.parametrize('R', [4., 10.])
def test_percepts_are_the_rules_on_the_six_plans(R, cone):
    sc = _six()['core'].scenery
    w = plan_percepts()
    assert all(np.array_equal(a, b) for a, b in zip(_walls(sc), w.walls))
    for K in (0, 1, 4, 16):
        seen = _call(sc, w, R, K, cone)
        assert seen.visible.dtype == torch.uint8 and seen.counts.dtype == seen.nearest.dtype == torch.int32 and seen.nearest.shape == (6, 2, K)
        same(_result(seen), plan_rule(R, cone, K))


def test_a_large_plan_whose_kept_walls_overflow_the_lds():
    from megastep_amd import cuda, scene
    geoms = plans(1, large=True)
    walls = np.asarray(geoms[0]['walls'], F).reshape(-1, 4)
    R = 10.
    lo, hi = np.minimum(walls[:, :2], walls[:, 2:]), np.maximum(walls[:, :2], walls[:, 2:])
    sp = spawn_points(geoms[0])
    kept = np.array([((lo <= p + F(R)) & (hi >= p - F(R))).all(1).sum() for p in sp])     # (a box inside the kernel's: at least these are kept)
    assert kept.max() > cuda.VIEW_WALL_CAPACITY
    eyes = np.stack([sp[kept.argmax()], sp[kept.argmin()], sp[len(sp)//2]])[None].astype(F)
    ends = np.concatenate([walls[:, :2], walls[:, 2:]])
    points = np.random.RandomState(4).uniform(ends.min(0), ends.max(0), (1, 200, 2)).astype(F)
    sc = scene.scenery(geoms, 1, device='cuda', bake=False)
    seen = cuda.percepts(sc, _dev(points), eyes=_dev(eyes), max_range=R, k=16)
    want = percept_rule.call(_walls(sc), eyes, points, R, 16)
    same(_result(seen), want)
    assert (want['counts'] > 0).all() and (want['counts'] < 200).all()
    print('kept walls: at least', int(kept.max()), 'of', len(walls), '- visible points:', want['counts'].reshape(-1).tolist())


_BOX = []


def _box():
    """box_walls() as a scenery of one agent, the NaN row put in afterwards."""
    if not _BOX:
        from megastep_amd import scene
        walls = hand_shape(1, 1).walls[0].copy()
        nan_row = np.flatnonzero(np.isnan(walls).any(1))
        walls[nan_row] = (1, 1, 3, 3)
        sc = scene.scenery([dict(walls=walls.reshape(-1, 2, 2), lights=np.array([[1., 1.]]))], 1, device='cuda', bake=False)
        af = sc.model.shape[0]
        sc.lines.vals[int(sc.lines.starts[0]) + af + int(nan_row[0])] = torch.tensor([[float('nan'), 1.], [3., float('nan')]], device='cuda')
        assert np.array_equal(_walls(sc)[0], hand_shape(1, 1).walls[0], equal_nan=True)
        _BOX.append(sc)
    return _BOX[0]


@pytest.mark.parametrize('P', [1, 63, 64, 65, 200, 1024])
@pytest.mark.parametrize('E', [1, 4, 5, 64])
def test_shapes_round_the_wave_and_the_workgroup(E, P):
    sc, w = _box(), hand_shape(E, P)
    for K, cone, gated in ((16, False, False), (1, True, True), (0, True, False)):
        kw = dict(valid=w.valid, pairs=w.pairs if K == 1 else w.pairs[None].copy()) if gated else {}
        rule_kw = dict(headings=w.headings, cos_half=w.cos_half) if cone else {}
        same(_result(_call(sc, w, 6., K, cone, **kw)), percept_rule.call(w.walls, w.eyes, w.points, 6., K, **rule_kw, **kw))


@pytest.mark.parametrize('cone', [False, True])
def test_a_point_is_seen_exactly_when_the_view_fields_see_the_cell_it_is_the_centre_of(cone):
    from megastep_amd import cuda
    c = _six()['core']
    grid = cuda.nav_grid(c.scenery, clearance=RADIUS)
    v = plan_views()
    eyes, headings = _dev(v.points), _dev(v.headings)
    kw = dict(headings=headings, fov=CONE) if cone else {}
    draws = cuda.cell_draws(grid, grid, 1, 64, seed=3)
    points = draws.points[:, 0].contiguous()
    assert (draws.cells >= 0).all()
    views = cuda.view_fields(grid, c.scenery, eyes, 10., **kw)
    seen = cuda.percepts(c.scenery, points, eyes=eyes, max_range=10., k=0, fields=('visible',), **kw)
    starts = torch.as_tensor(grid._host_starts[:-1], device='cuda')[:, None, None]
    sizes = torch.as_tensor(grid._host_starts[1:] - grid._host_starts[:-1], device='cuda')[:, None, None]
    store = 2*starts + torch.arange(2, device='cuda')[None, :, None]*sizes + draws.cells[:, 0][:, None, :].long()
    assert torch.equal(seen.visible, views.values[store.reshape(-1)].reshape(6, 2, 64))
    assert 0 < int(seen.visible.sum()) < seen.visible.numel()


def test_fields_out_a_mask_from_the_device_and_a_side_stream():
    from megastep_amd import cuda
    sc = _six()['core'].scenery
    w = plan_percepts()
    want = plan_rule(10., True, 4)
    points, eyes, headings = _dev(w.points), _dev(w.eyes), _dev(w.headings)
    # fields= subsets: the others are not there
    for fields in (('counts',), ('nearest', 'near_distances'), ('visible', 'squares', 'offsets'), ('near_offsets',)):
        seen = cuda.percepts(sc, points, eyes=eyes, headings=headings, fov=CONE, max_range=10., k=4, fields=fields)
        assert all((getattr(seen, k) is not None) == (k in fields) for k in KEYS)
        same(_result(seen), want, fields)
    # out= rewrites in place, with the same data pointers; a mask from a device tensor keeps the other rows
    seen = cuda.percepts(sc, points, eyes=eyes, headings=headings, fov=CONE, max_range=4., k=4)
    first = _result(seen)
    same(first, plan_rule(4., True, 4))
    ptrs = [t.data_ptr() for t in seen._t]
    mask = torch.as_tensor(np.random.RandomState(6).rand(6, 2) < .5, device='cuda')
    mask[0, 0], mask[0, 1] = True, False
    again = cuda.percepts(sc, points, eyes=eyes, headings=headings, fov=CONE, max_range=10., k=4, mask=mask, out=seen)
    assert again is seen and [t.data_ptr() for t in seen._t] == ptrs
    same(_result(seen), percept_rule.call(w.walls, w.eyes, w.points, 10., 4, headings=w.headings, cos_half=w.cos_half, mask=_np(mask), before=first))
    assert not np.array_equal(_np(seen.counts), first['counts'])
    for kw in (dict(k=3), dict(fields=('counts',)), dict(points=points[:, :100].contiguous()), dict(eyes=eyes[:, :1].contiguous(), headings=headings[:, :1].contiguous())):
        with pytest.raises(RuntimeError, match='`out` must come from a percepts call'):
            cuda.percepts(sc, **{**dict(points=points, eyes=eyes, headings=headings, fov=CONE, max_range=10., k=4), **kw}, out=seen)
    with pytest.raises(RuntimeError, match='`out` must come from a percepts call'):
        cuda.percepts(sc, points, eyes=eyes, max_range=10., k=4, out=seen)       # (without the cone)
    # a side stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        cuda.percepts(sc, points, eyes=eyes, headings=headings, fov=CONE, max_range=10., k=4, out=seen)
    side.synchronize()
    same(_result(seen), want)


def _agents_rule(c, seen, R, K, cos_half):
    """percept_rule on the agents as they stand: eyes and points their positions, everyone but itself, the headings the call made."""
    a = c.n_agents
    positions = _np(c.agents.positions)
    walls = _walls(c.scenery)
    return percept_rule.call(walls, positions, positions, R, K, headings=_np(seen.headings), cos_half=cos_half, pairs=1 - np.eye(a, dtype=np.uint8))


def test_the_agents_form_in_a_graph_replayed_three_times():
    from megastep_amd import cuda
    from tests.test_navview_host import cos_half_of
    c = _six()['core']
    agents = c.agents
    held = agents.positions.clone(), agents.angles.clone()
    try:
        seen = cuda.percepts(c.scenery, agents=agents, fov=CONE, k=1)
        assert seen.eyes is agents.positions and seen.points is agents.positions and seen.visible.shape == (6, 2, 2)
        deg = _np(agents.angles).astype(np.float64)
        assert np.allclose(_np(seen.headings), np.stack([np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))], -1), atol=1e-6)
        same(_result(seen), _agents_rule(c, seen, 10., 1, cos_half_of(CONE)))
        assert not _np(seen.visible)[:, [0, 1], [0, 1]].any()             # (nobody looks at itself)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            cuda.percepts(c.scenery, agents=agents, fov=CONE, k=1, out=seen)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            cuda.percepts(c.scenery, agents=agents, fov=CONE, k=1, out=seen)
        counts = []
        for replay in range(3):
            if replay:
                agents.positions[:, 1] += torch.tensor([-.4, .25], device='cuda')
                agents.angles[:] = agents.angles + 70.
            graph.replay()
            got = _result(seen)
            eager = cuda.percepts(c.scenery, agents=agents, fov=CONE, k=1)
            same(got, _result(eager))
            same(got, _agents_rule(c, seen, 10., 1, cos_half_of(CONE)))
            counts.append(got['visible'].copy())
        assert not np.array_equal(counts[0], counts[1]) or not np.array_equal(counts[1], counts[2])
    finally:
        agents.positions.copy_(held[0])
        agents.angles.copy_(held[1])


def _packed(want, angles, R):
    """modules.Percepts.pack in numpy, binary32: to_local_frame's arithmetic with numpy's sine and cosine."""
    a = (np.float32(np.pi/180)*angles.astype(F))[..., None]
    s, c = np.sin(a), np.cos(a)
    x, y = want['near_offsets'][..., 0], want['near_offsets'][..., 1]
    rows = np.stack([np.ones_like(x), (c*x + s*y)/F(R), (-s*x + c*y)/F(R), want['near_distances']/F(R)], -1)
    listed = np.arange(x.shape[-1]) < want['counts'][..., None]
    return np.where(listed[..., None], rows, F(0)).astype(F)


def test_the_percepts_module_is_the_rules_planes_packed():
    from megastep_amd import modules
    from tests.test_navview_host import cos_half_of
    c = _six()['core']
    # the other agents
    module = modules.Percepts(c, max_range=10., fov=CONE, k=1)
    obs = module()
    want = _agents_rule(c, module.reading, 10., 1, cos_half_of(CONE))
    assert obs.shape == (6, 2, 1, 4) == (6,) + module.space.shape and module.reading.visible is None
    assert np.allclose(_np(obs), _packed(want, _np(c.agents.angles), 10.), atol=1e-6) and not np.isnan(_np(obs)).any()
    assert (_np(obs)[..., 0] == (want['counts'] > 0)[..., None]).all()
    # points of one's own, without a cone; the module keeps its buffers
    w = plan_percepts()
    module = modules.Percepts(c, points=_dev(w.points), max_range=4., k=4)
    obs = module()
    positions = _np(c.agents.positions)
    want = percept_rule.call(w.walls, positions, w.points, 4., 4)
    assert np.allclose(_np(obs), _packed(want, _np(c.agents.angles), 4.), atol=1e-6)
    assert 0 < (want['counts'] > 0).sum() and (_np(obs)[..., 0].sum(-1) == np.minimum(want['counts'], 4)).all()
    reading = module.reading
    module()
    assert module.reading is reading


_TAG = {}


def _tag(graphed):
    from megastep_amd import graphs
    from megastep_amd.demo import Tag
    torch.manual_seed(3); np.random.seed(3)
    if 'geoms' not in _TAG:
        _TAG['geoms'] = plans(64)
    env = Tag(64, 2, 2, geometries=_TAG['geoms'], tag_range=3., max_lifespan=10**6)
    return env, (graphs.GraphedStep(env, warmup=3) if graphed else env)


def _actions(t):
    return torch.as_tensor(np.random.RandomState(100 + t).randint(0, 7, (64, 4)), device='cuda')


def test_tag_as_one_hip_graph_equals_the_eager_env_key_for_key():
    from megastep_amd import arrdict
    logs = []
    for graphed in (False, True):
        env, stepper = _tag(graphed)
        stepper.reset()
        log = []
        # the graphed env's first step call is four steps: three of warm-up and the captured one, all under the first actions
        for t in range(30 if graphed else 33):
            world = stepper.step(arrdict.arrdict(actions=_actions(t if graphed else max(t - 3, 0))))
            log.append({**{k: v.clone() for k, v in world.obs.items()}, 'reward': world.reward.clone(), 'reset': world.reset.clone(),
                        'positions': env.core.agents.positions.clone(), 'tagged': env._tagged.clone()})
        logs.append(log)
    eager, graphed = logs
    assert sorted(graphed[0]) == ['d', 'percepts', 'positions', 'reset', 'reward', 'rgb', 'role', 'tagged']
    assert graphed[0]['percepts'].shape == (64, 4, 3, 4) and graphed[0]['role'].shape == (64, 4, 1)
    for k in range(30):
        for key in graphed[k]:
            assert torch.equal(graphed[k][key], eager[k + 3][key]), (k, key)
    assert sum(int(step['tagged'].sum()) for step in graphed) > 0 and sum(float(step['reward'].abs().sum()) for step in graphed) > 0
    assert not torch.equal(graphed[0]['positions'], graphed[-1]['positions'])


def test_tag_books_read_a_percepts_call_and_a_tagged_hider_starts_over_on_a_free_cell():
    from megastep_amd import arrdict, cuda
    from megastep_amd.demo import Tag
    env, _ = _tag(False)
    env.reset()
    c, grid = env.core, env.grid
    eye = 1 - torch.eye(4, dtype=torch.uint8, device='cuda')
    geom, starts = torch.as_tensor(grid._host_geom, device='cuda'), torch.as_tensor(grid._host_starts[:-1], device='cuda')
    respawned = 0
    for t in range(30):
        tagged = env._tagged.clone()
        world = env.step(arrdict.arrdict(actions=_actions(t)))
        # the game's inputs: a percepts call made by hand on the same poses
        positions, angles = c.agents.positions, c.agents.angles
        radians = angles*(np.pi/180)
        headings = torch.stack([torch.cos(radians), torch.sin(radians)], -1)
        fresh = cuda.percepts(c.scenery, positions.clone(), eyes=positions.clone(), headings=headings, fov=c.fov, max_range=env.sight, k=3, pairs=eye)
        same(_result(env.seen), _result(fresh))
        reward, now = Tag.books(fresh.visible, fresh.squares, env.roles, env.tag_range, env.hide_bonus)
        assert torch.equal(world.reward, reward) and torch.equal(env._tagged, now) and not now[:, :2].any()
        assert not world.reset.any()
        # who was tagged at the last step stands on the centre of a free cell now
        if tagged.any():
            n, a = tagged.nonzero(as_tuple=True)
            at = positions[n, a]
            j = torch.floor(at[:, 0]/grid.cell).long() - geom[n, 0]
            i = torch.floor(at[:, 1]/grid.cell).long() - geom[n, 1]
            assert ((j >= 0) & (j < geom[n, 2]) & (i >= 0) & (i < geom[n, 3])).all()
            assert (grid.free[starts[n] + i*geom[n, 2] + j] == 1).all()
            centre = torch.stack([((geom[n, 0] + j).float() + .5)*grid.cell, ((geom[n, 1] + i).float() + .5)*grid.cell], -1)
            assert torch.equal(at, centre) and (c.agents.velocity[n, a] == 0).all()
            respawned += len(n)
    assert respawned > 0


def test_the_tag_expert_runs_without_a_nan():
    env, _ = _tag(False)
    env.reset()
    start = env.core.agents.positions.clone()
    for t in range(30):
        decision = env.expert()
        assert decision.actions.shape == (64, 4) and decision.actions.dtype == torch.int64
        assert ((decision.actions >= 0) & (decision.actions <= 6)).all()
        world = env.step(decision)
        assert torch.isfinite(world.reward).all() and torch.isfinite(world.obs.percepts).all() and torch.isfinite(env.core.agents.positions).all()
    moved = (env.core.agents.positions - start).norm(dim=-1)
    assert (moved[:, :2] > .5).any() and (moved[:, 2:] > .5).any()
