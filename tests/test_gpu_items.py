"""Items on the GPU (cuda.collect_items, cuda.place_items, cuda.overlay_items, modules.Items, demo.Forage): the two kernels are held
to EQUALITY with their host instantiations - which the CPU suite holds to tests/item_rule.py - as bits, at the shapes round a
wave's 64 items and a workgroup's 256 rays; the overlay on real renders and casts; the return step in a replayed graph; then
what is built on them."""
import numpy as np
import pytest
import torch

from tests import item_rule as ir
from tests.item_rule import COLLECT_KEYS, F, OVERLAY_KEYS
from tests.test_navfield_host import plans
from tests.test_gpu_navseen import _core, _np
from tests.test_gpu_navview import _walls

pytestmark = pytest.mark.gpu

_KEPT = {}


def _dev(a, dtype=None):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), device='cuda', dtype=dtype)


def _box(A):
    """The hand-made world's box as a scenery of A agents, its NaN row put in behind the builder's back; and agents to pose."""
    from megastep_amd import core, cuda, scene
    if ('box', A) not in _KEPT:
        walls = ir.hand_items(1, 1).walls[0].copy()
        nan_row = np.flatnonzero(np.isnan(walls).any(1))
        walls[nan_row] = (1, 1, 3, 3)
        sc = scene.scenery([dict(walls=walls.reshape(-1, 2, 2), lights=np.array([[1., 1.]]))], A, device='cuda', bake=False)
        af = A*sc.model.shape[0]
        sc.lines.vals[int(sc.lines.starts[0]) + af + int(nan_row[0])] = torch.tensor([[float('nan'), 1.], [3., float('nan')]], device='cuda')
        assert np.array_equal(_walls(sc)[0], ir.hand_items(1, 1).walls[0], equal_nan=True)
        cuda.initialize(core.AGENT_RADIUS, 64, 130, 10)
        _KEPT['box', A] = (sc, core._init_agents(1, A, 'cuda'))
    return _KEPT['box', A]


def _store(w, n_kinds, envs=slice(None)):
    from megastep_amd import cuda
    return cuda.Items(_dev(w.positions[envs]), _dev(w.timers[envs]), _dev(w.kinds[envs]), _dev(w.colors[envs]), n_kinds)


def _collected(store, got):
    return dict(positions=_np(store.positions), timers=_np(store.timers), taker=_np(got.taker), counts=_np(got.counts),
                due=_np(got.due).astype(np.uint8))


@pytest.mark.parametrize('P,A', [(1, 1), (63, 4), (64, 4), (65, 64), (1024, 4), (1024, 64)])
def test_the_collect_kernel_is_its_host_statement_on_the_hand_made_world(P, A):
    from megastep_amd import cuda
    sc, agents = _box(A)
    w = ir.hand_items(P, A)
    agents.positions.copy_(_dev(w.agents))
    for kw in (dict(delay=3), dict(delay=-1, takers=w.takers), dict(delay=0, through_walls=True), dict(reset=np.ones(1, np.uint8))):
        store = _store(w, 8)
        got = cuda.collect_items(sc, agents, store, .35, **{k: _dev(v) if isinstance(v, np.ndarray) else v for k, v in kw.items()})
        assert got.taker.dtype == got.counts.dtype == torch.int32 and got.due.dtype == torch.bool and got.counts.shape == (1, A, 8)
        ir.same(_collected(store, got), ir.host_collect(w.walls, w.agents, w.positions, w.timers, w.kinds, 8, .35, **kw), COLLECT_KEYS)


def _plan_world(P=256, A=3, per=200):
    """Five of the six plans with A agents posed as plan_items() has them."""
    if ('plans', P, A, per) not in _KEPT:
        w = ir.plan_items(P, A, per)
        c = _core((plans(3) + plans(3, oblique=True))[:5], A, 64)
        assert all(np.array_equal(a, b) for a, b in zip(_walls(c.scenery), w.walls[:5]))
        c.agents.positions.copy_(_dev(w.agents[:5]))
        _KEPT['plans', P, A, per] = (c, w)
    return _KEPT['plans', P, A, per]


def test_the_collect_kernel_is_its_host_statement_on_the_plans():
    from megastep_amd import cuda
    c, w = _plan_world()
    for through in (False, True):
        store = _store(w, 3, slice(0, 5))
        got = cuda.collect_items(c.scenery, c.agents, store, .5, delay=2, through_walls=through)
        want = ir.host_collect(w.walls[:5], w.agents[:5], w.positions[:5], w.timers[:5], w.kinds[:5], 3, .5, delay=2, through_walls=through)
        ir.same(_collected(store, got), want, COLLECT_KEYS)
        assert (want['taker'] >= 0).sum() > 20


def _planes(frame):
    return {k: _np(getattr(frame, k)).reshape((frame.distances.shape[0], -1) + ((3,) if k == 'screen' else ()))
            for k in ir.PLANES if getattr(frame, k, None) is not None}


def _overlaid(frame):
    return {**_planes(frame), 'items': _np(frame.items).reshape(frame.items.shape[0], -1)}


def test_the_overlay_kernel_is_its_host_statement_at_the_largest_shape_and_with_an_env_without_items():
    """5 envs x 3 agents x 200 rays x 256 items over the planes of a cast at the walls; env 2 holds no present item."""
    from megastep_amd import cuda
    c, w = _plan_world()
    positions = w.positions[:5].copy()
    positions[2] = np.nan
    store = cuda.Items(_dev(positions), _dev(w.timers[:5]), _dev(w.kinds[:5]), _dev(w.colors[:5]), 3)
    origins, dirs = _dev(w.agents[:5]), _dev(w.dirs[:5])
    each = origins.repeat_interleave(200, 1).contiguous()
    cast = cuda.raycast(c.scenery, each, dirs, near=.1, fields=('indices', 'locations', 'dots', 'distances'))
    before = _planes(cast)
    widths = _np(c.scenery.lines.widths)
    want = ir.host_overlay(positions, w.colors[:5], w.agents[:5], w.dirs[:5], .1, .1, widths, before)
    cuda.overlay_items(store, cast, origins=origins, dirs=dirs, near=.1)
    got = _overlaid(cast)
    ir.same(got, want, [k for k in OVERLAY_KEYS if k != 'screen'])
    assert (got['items'][2] == -1).all() and np.array_equal(ir.bits(got['distances'][2]), ir.bits(before['distances'][2]))
    assert 500 < (got['items'] >= 0).sum() < got['items'].size - 500


@pytest.mark.parametrize('P', [1, 64, 65, 256])
@pytest.mark.parametrize('per', [1, 37, 64, 65, 200])
def test_the_overlay_kernel_is_its_host_statement_on_the_hand_made_world(per, P):
    from megastep_amd import cuda
    sc, agents = _box(3)
    w = ir.hand_items(P, 3)
    dirs = np.concatenate([ir.ring(per, phase=.37*a) for a in range(3)])[None]
    each = np.repeat(w.agents, per, 1)
    cast = cuda.raycast(sc, _dev(each), _dev(dirs), near=.1, fields=('indices', 'locations', 'dots', 'distances'))
    want = ir.host_overlay(w.positions, w.colors, w.agents, dirs, .1, .1, _np(sc.lines.widths), _planes(cast))
    cuda.overlay_items(_store(w, 8), cast, origins=_dev(w.agents), dirs=_dev(dirs), near=.1)
    ir.same(_overlaid(cast), want, [k for k in OVERLAY_KEYS if k != 'screen'])


@pytest.mark.parametrize('P', [257, 512, 1023, 1024])
@pytest.mark.parametrize('per', [255, 256, 257, 600])
def test_the_overlay_kernel_past_one_window_of_items_and_one_chunk_of_rays(per, P):
    """item_overlay_kernel's compaction loop run two to four times (`kept` carried from window to window) and its rays in one to
    three chunks, over item_rule.wide_items()' sets - whose counts, window by window, tests/test_item_host.py asserts and holds to
    the rule; the host statement compacts serially and takes an origin's rays in one go."""
    from megastep_amd import cuda
    sc, agents = _box(3)
    dirs = np.concatenate([ir.ring(per, phase=.37*a) for a in range(3)])[None]
    chunks = -(-per//ir.OVERLAY_WINDOW)
    for which in ir.WIDE_SETS:
        w = ir.wide_items(P, which)
        ir.check_wide(w, which)
        each = np.repeat(w.agents, per, 1)
        cast = cuda.raycast(sc, _dev(each), _dev(dirs), near=.1, fields=('indices', 'locations', 'dots', 'distances'))
        want = ir.host_overlay(w.positions, w.colors, w.agents, dirs, ir.WIDE_RADIUS, .1, _np(sc.lines.widths), _planes(cast))
        cuda.overlay_items(_store(w, 8), cast, origins=_dev(w.agents), dirs=_dev(dirs), near=.1, radius=ir.WIDE_RADIUS)
        got = _overlaid(cast)
        ir.same(got, want, [k for k in OVERLAY_KEYS if k != 'screen'])
        shown = (got['items'] >= 0).reshape(3, per)
        assert shown.any() and not shown.all(), which
        # the rays of the last chunk (('late', 257): one item in all)
        assert shown[:, (chunks - 1)*ir.OVERLAY_WINDOW:].any() or (which, P) == ('late', 257), which
        if which == 'late':
            assert got['items'][shown.reshape(1, -1)].min() >= ir.OVERLAY_WINDOW


def test_the_overlay_kernel_in_three_chunks_beside_an_env_without_items():
    """5 envs x 3 agents x 600 rays x 512 items: every origin's rays in three workgroups, each of which compacts two windows of
    items; env 2 holds no present item (`kept == 0` in all three chunks of its origins)."""
    from megastep_amd import cuda
    c, w = _plan_world(512, 3, 600)
    positions = w.positions[:5].copy()
    positions[2] = np.nan
    for n in (0, 1, 3, 4):
        assert all(ir.overlay_windows(positions[n], o)[1] > 0 for o in w.agents[n])
    assert sum(ir.overlay_windows(positions[2], w.agents[2, 0])) == 0
    store = cuda.Items(_dev(positions), _dev(w.timers[:5]), _dev(w.kinds[:5]), _dev(w.colors[:5]), 3)
    origins, dirs = _dev(w.agents[:5]), _dev(w.dirs[:5])
    cast = cuda.raycast(c.scenery, origins.repeat_interleave(600, 1).contiguous(), dirs, near=.1,
                        fields=('indices', 'locations', 'dots', 'distances'))
    before = _planes(cast)
    want = ir.host_overlay(positions, w.colors[:5], w.agents[:5], w.dirs[:5], .1, .1, _np(c.scenery.lines.widths), before)
    cuda.overlay_items(store, cast, origins=origins, dirs=dirs, near=.1)
    got = _overlaid(cast)
    ir.same(got, want, [k for k in OVERLAY_KEYS if k != 'screen'])
    assert (got['items'][2] == -1).all() and np.array_equal(ir.bits(got['distances'][2]), ir.bits(before['distances'][2]))
    last = (got['items'] >= 0).reshape(5, 3, 600)[:, :, 2*ir.OVERLAY_WINDOW:]
    assert last[[0, 1, 3, 4]].any((-1, -2)).all() and (got['items'] >= ir.OVERLAY_WINDOW).any()         # (every env's last chunks)


@pytest.mark.parametrize('res', [64, 37])
def test_the_overlay_on_a_real_render(res):
    """5 envs x 3 agents x res rays: every plane of the Render, screen included, and the items plane."""
    from megastep_amd import cuda
    _, w = _plan_world()
    if ('render', res) not in _KEPT:
        c = _core((plans(3) + plans(3, oblique=True))[:5], 3, res)
        c.agents.positions.copy_(_dev(w.agents[:5]))
        _KEPT['render', res] = c
    c = _KEPT['render', res]
    store = _store(w, 3, slice(0, 5))
    frame = cuda.render(c.scenery, c.agents)
    before = _planes(frame)
    dirs = cuda.camera_rays(c.agents)
    want = ir.host_overlay(w.positions[:5], w.colors[:5], w.agents[:5], _np(dirs).reshape(5, -1, 2), .1, c.agent_radius,
                           _np(c.scenery.lines.widths), before)
    assert cuda.overlay_items(store, frame, agents=c.agents) is frame and frame.items.shape == (5, 3, res) and frame.items.dtype == torch.int32
    got = _overlaid(frame)
    ir.same(got, want, OVERLAY_KEYS)
    shown = got['items'] >= 0
    assert 30 < shown.sum() < shown.size - 30
    # an item's ray is no line of the env: shade leaves it black, the overlay's colour is the item's own
    assert (got['indices'][shown] >= _np(c.scenery.lines.widths)[:, None].repeat(3*res, 1)[shown]).all()
    # a body nearer than the item hides it: where the render saw an agent, an item is shown only if it is nearer
    bodies = (before['indices'] >= 0) & (before['indices'] < 3*c.scenery.model.shape[0])
    assert (got['distances'][bodies & shown] < before['distances'][bodies & shown]).all()


def test_the_overlay_on_a_ring_of_cast_rays_with_out_and_a_side_stream():
    """A cast's rays, an origin a ray, the agents' bodies in the planes; `out_items=`; and the same launch on a side stream."""
    from megastep_amd import cuda
    c, w = _plan_world()
    rng = np.random.RandomState(9)
    origins = np.repeat(w.agents[:5, :1] + rng.uniform(-.2, .2, (5, 1, 2)).astype(F), 96, 1).astype(F)
    origins[:, 48:] = np.repeat(w.agents[:5, 1:2], 48, 1) + F(.05)
    dirs = np.stack([np.concatenate([ir.ring(48, .1*n), ir.ring(48, .5 + .1*n)]) for n in range(5)])
    store = _store(w, 3, slice(0, 5))
    results = []
    for stream in (None, torch.cuda.Stream()):
        if stream is not None:
            stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            cast = cuda.raycast(c.scenery, _dev(origins), _dev(dirs), agents=c.agents, near=.1)
            before = _planes(cast)
            shown = torch.full((5, 96), -9, dtype=torch.int32, device='cuda')
            cuda.overlay_items(store, cast, origins=_dev(origins), dirs=_dev(dirs), near=.1, out_items=shown)
            assert cast.items is shown
        if stream is not None:
            torch.cuda.current_stream().wait_stream(stream)
        results.append(_overlaid(cast))
    want = ir.host_overlay(w.positions[:5], w.colors[:5], origins, dirs, .1, .1, _np(c.scenery.lines.widths), before)
    for got in results:
        ir.same(got, want, [k for k in OVERLAY_KEYS if k != 'screen'])
    assert (want['items'] >= 0).sum() > 30


def test_collect_draw_and_place_in_a_graph_replayed_three_times():
    """Every replay empties the envs' stores (reset), so every item is due, drawn afresh and placed on a free cell."""
    from megastep_amd import cuda
    c, _ = _plan_world()
    grid = cuda.nav_grid(c.scenery, config=c.config)
    store = cuda.items(5, 40, kinds=torch.arange(40) % 2)
    reset = torch.ones(5, dtype=torch.bool, device='cuda')
    collected = cuda.collect_items(c.scenery, c.agents, store, .3, reset=reset)
    assert collected.due.all() and not store.present().any()
    draws = cuda.cell_draws(grid, grid, 40, 1, seed=5, mask=collected.due)
    cuda.place_items(store, draws, collected.due)
    assert store.present().all()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert cuda.collect_items(c.scenery, c.agents, store, .3, reset=reset, out=collected) is collected
        cuda.place_items(store, draws, collected.due)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cuda.collect_items(c.scenery, c.agents, store, .3, reset=reset, out=collected)
        cuda.place_items(store, draws, collected.due)
    free, starts = _np(grid.free), grid._host_starts
    seen = []
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert collected.due.all() and store.present().all() and (collected.counts == 0).all()
        cells, points = _np(draws.cells)[:, :, 0], _np(draws.points)[:, :, 0]
        assert (cells >= 0).all() and np.array_equal(_np(store.positions), points)
        assert all((free[starts[n] + cells[n]] & 1).all() for n in range(5))
        seen.append(points.copy())
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2]) and not np.array_equal(seen[0], seen[2])
    # an item whose draw finds no cell stays absent with timer 0 and is due again: a gate that lets nothing through
    shut = cuda.cell_layer(torch.zeros_like(grid.free))
    nowhere = cuda.cell_draws(grid, grid, 40, 1, gate=shut, seed=5)
    for call in range(2):
        cuda.collect_items(c.scenery, c.agents, store, .3, reset=reset if call == 0 else None, out=collected)
        cuda.place_items(store, nowhere, collected.due)
        assert collected.due.all() and not store.present().any() and (store.timers == 0).all()


def _forage(n_envs, graphed=False, **kw):
    from megastep_amd import graphs
    from megastep_amd.demo import Forage
    torch.manual_seed(3); np.random.seed(3)
    if 'geoms' not in _KEPT:
        _KEPT['geoms'] = plans(64)
    env = Forage(n_envs, geometries=_KEPT['geoms'][:n_envs], **kw)
    return env, (graphs.GraphedStep(env, warmup=3) if graphed else env)


def _actions(t, n):
    return torch.as_tensor(np.random.RandomState(100 + t).randint(0, 7, (n, 2)), device='cuda')


def test_forage_as_one_hip_graph_equals_the_eager_env_key_for_key():
    from megastep_amd import arrdict
    logs = []
    for graphed in (False, True):
        env, stepper = _forage(16, graphed, n_agents=2, n_items=24, values=(1., -1.), colors=[(1., 0., 0.), (0., 1., 0.)]*12, delay=2,
                               reach=.6, max_lifespan=10**6)      # (lifespans out of reach: no step draws random numbers)
        stepper.reset()
        log = []
        # the graphed env's first step call is four steps: three of warm-up and the captured one, all under the first actions
        for t in range(8 if graphed else 11):
            world = stepper.step(arrdict.arrdict(actions=_actions(t if graphed else max(t - 3, 0), 16)))
            log.append({**{k: v.clone() for k, v in world.obs.items()}, 'reward': world.reward.clone(), 'reset': world.reset.clone(),
                        'positions': env.core.agents.positions.clone(), 'items': env.items.positions.clone(), 'shown': env.frame.items.clone()})
        logs.append(log)
    eager, graphed = logs
    assert sorted(graphed[0]) == ['d', 'items', 'percepts', 'positions', 'reset', 'reward', 'rgb', 'shown']
    assert graphed[0]['percepts'].shape == (16, 2, 4, 4) and graphed[0]['rgb'].shape == (16, 2, 3, 1, 64) and graphed[0]['shown'].shape == (16, 2, 256)
    for k in range(8):
        for key in graphed[k]:
            assert torch.equal(graphed[k][key], eager[k + 3][key]) or \
                (graphed[k][key].dtype.is_floating_point and np.array_equal(ir.bits(_np(graphed[k][key])), ir.bits(_np(eager[k + 3][key])))), (k, key)
    assert any(bool((step['shown'] >= 0).any()) for step in graphed)
    assert not torch.equal(graphed[0]['positions'], graphed[-1]['positions'])


def test_forage_draws_the_items_of_an_env_anew_when_an_episode_ends():
    from megastep_amd import arrdict
    env, _ = _forage(8, n_items=12, max_lifespan=4, delay=-1)
    world = env.reset()
    assert bool(world.reset.all()) and bool(env.items.store.present().all()) and world.reward.shape == (8, 1)
    renewed = 0
    for t in range(10):
        before = env.items.positions.clone()
        world = env.step(arrdict.arrdict(actions=_actions(t, 8)[:, :1]))
        assert world.obs.rgb.shape == (8, 1, 3, 1, 64) and world.obs.d.shape == (8, 1, 1, 1, 64) and world.obs.percepts.shape == (8, 1, 4, 4)
        fresh = world.reset
        if bool(fresh.any()):
            assert bool(env.items.store.present()[fresh].all()) and not torch.equal(env.items.positions[fresh], before[fresh])
            renewed += int(fresh.sum())
        # (delay = -1: outside a reset an item that is there stays where it is or is taken for good)
        kept = env.items.store.present()[~fresh]
        assert torch.equal(env.items.positions[~fresh][kept], before[~fresh][kept])
    assert renewed > 0


def test_the_expert_collects_more_than_random_actions():
    """Forage(64), 300 steps: the totals under expert() and under random actions. Measured on an MI355X: see DESIGN.md 3.34."""
    from megastep_amd import arrdict
    totals = {}
    for who in ('expert', 'random'):
        env, _ = _forage(64, n_items=16, max_lifespan=10**6)
        env.reset()
        total = torch.zeros((), device='cuda')
        rng = np.random.RandomState(7)
        for t in range(300):
            decision = env.expert() if who == 'expert' else arrdict.arrdict(actions=torch.as_tensor(rng.randint(0, 7, (64, 1)), device='cuda'))
            total += env.step(decision).reward.sum()
        totals[who] = float(total)
    print(f'items collected in 300 steps of Forage(64): expert {totals["expert"]:.0f}, random {totals["random"]:.0f}')
    assert totals['expert'] > totals['random']
