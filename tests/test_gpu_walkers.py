"""Walkers on the GPU: walker_kernel - both instantiations - held to EQUALITY with its host instantiation, which the CPU suite holds
to walk_rule, in the whole store and every record, floats by their bits; then what is built on it (demo.Crowd, the overlay)."""
import numpy as np
import pytest
import torch

from tests import walker_rule as wr
from tests.walker_rule import KEYS, NAN
from tests.item_rule import bits
from tests.test_navfield_host import RADIUS as AGENT_RADIUS, plans
from tests.test_gpu_navseen import _core, _np
from tests.test_gpu_navview import _walls

pytestmark = pytest.mark.gpu


_dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device='cuda')


def _world(geoms, A, P, seed, bake=True, fast=None):
    """The plans as a scenery (`bake`: with a wall grid), A agents at random in their boxes, wr.random_store() there and on the device."""
    from megastep_amd import core, cuda, scene
    sc = scene.scenery(geoms, A, device='cuda', bake=bake, random=np.random.RandomState(seed))
    agents, walls, N = core._init_agents(len(geoms), A, 'cuda'), _walls(sc), len(geoms)
    agents._config = cuda.config(core.AGENT_RADIUS, 64, 130, 10)
    lo, hi = [w.reshape(-1, 2).min(0) for w in walls], [w.reshape(-1, 2).max(0) for w in walls]
    rng = np.random.RandomState(seed)
    agents.positions.copy_(_dev(np.stack([rng.uniform(lo[n], hi[n], (A, 2)) for n in range(N)]).astype(np.float32)))
    store, towards = wr.random_store(N, P, lo, hi, seed, fast)
    return sc, agents, walls, store, _dev(towards), cuda.walkers(N, P)


def _tick(sc, agents, walls, store, towards, dev, load=True, walk=None, **kw):
    """One tick on the device - cuda.walk, or `walk()` - and by the host statement from the numpy `store`, compared: the store after it."""
    from megastep_amd import core, cuda
    for k in wr.STORE + ('speeds',) if load else ():
        getattr(dev, k).copy_(_dev(store[k]))
    walked = walk() if walk else cuda.walk(sc, agents, dev, towards, **{k: _dev(v) if isinstance(v, np.ndarray) else v for k, v in kw.items()})
    torch.cuda.synchronize()
    want = wr.host_walk(walls, _np(agents.positions), store, _np(towards), radius=core.AGENT_RADIUS, **kw)
    wr.same({k: _np(getattr(dev if k in wr.STORE else walked, k)) for k in KEYS}, want, KEYS)
    return dict(store, **{k: want[k] for k in wr.STORE}), want


@pytest.mark.parametrize('N,bake', [(1, True), (5, True), (5, False)])
@pytest.mark.parametrize('A,P', [(1, 1), (5, 63), (1, 64), (5, 65), (1, 256), (5, 258), (1, 1024)])
def test_the_kernel_is_its_host_statement_in_both_instantiations(A, P, N, bake):
    """P up to 64: a wavefront an env - of five envs the last block holds one; beyond: a workgroup an env.  Two ticks; of five envs
    the fourth has no walker at all and the second is reset.  Slot 0 walks at 40 m/s: its reach is beyond what the wall grid's near
    lists cover, so it walks the env's rows while the lanes beside it walk their lists; slot 1 at 9 m/s takes the lists' long tier;
    every other slot the short one.  `bake=False`: a scenery without a wall grid, where every walker walks the env's rows."""
    sc, agents, walls, store, towards, dev = _world((plans(3) + plans(3, oblique=True))[:N], A, P, 7*A + P, bake, fast={0: 40., 1: 9.})
    reset, (lo, hi) = np.zeros(N, np.uint8), sc.WALL_GRID_REACH
    if N == 5:
        store['positions'][3], reset[1] = NAN, 1
    v = wr.host_walk([np.zeros((0, 4), np.float32)]*N, _np(agents.positions), store, _np(towards), keep=.3, radius=1e-6)['velocities'][0]
    reach = 1.02*(1.0102*np.linalg.norm(v, axis=-1)/10 + 2.002*AGENT_RADIUS) + 1e-3      # (nothing to meet there: the blend's own v; wall_reach)
    assert reach[0] > 1.05*hi and (P == 1 or .95*hi > reach[1] > 1.05*lo) and (P <= 2 or reach[2:].max() < .95*lo)
    for _ in range(2):
        store, want = _tick(sc, agents, walls, store, towards, dev, reset=reset, keep=.3)
    assert N == 1 or ((want['blocked'][[1, 3]] == 4).all() and (want['blocked'][[0, 2, 4]] < 4).any())
    assert P < 63 or ((want['blocked'] == 3).any() and (want['blocked'] == 2).any())


def test_sixteen_ticks_in_a_row_then_three_replays_of_a_graph():
    """Two plans, the store compared after every tick; `out=` on a side stream; then three replays, each a later tick."""
    from megastep_amd import cuda
    sc, agents, walls, store, towards, dev = _world(plans(3)[1:], 3, 40, 11)
    kw = dict(personal=.5, push=1.5, keep=.6)
    side, walked = torch.cuda.Stream(), None

    def eager():
        nonlocal walked
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            out = cuda.walk(sc, agents, dev, towards, out=walked, **kw)
        assert walked is None or out is walked
        walked = out
        return out

    for t in range(16):
        store, _ = _tick(sc, agents, walls, store, towards, dev, load=t == 0, walk=eager, **kw)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cuda.walk(sc, agents, dev, towards, out=walked, **kw)
    for t in range(3):
        store, want = _tick(sc, agents, walls, store, towards, dev, load=False, walk=lambda: graph.replay() or walked, **kw)
    assert np.isfinite(store['positions']).all(-1).any()


def test_crowd_as_one_hip_graph_equals_the_eager_env_key_for_key():
    from megastep_amd import arrdict, graphs
    from megastep_amd.demo import Crowd
    logs = []
    for graphed in (False, True):
        torch.manual_seed(3); np.random.seed(3)
        env = Crowd(16, n_walkers=12, geometries=plans(16), max_lifespan=10**6)
        stepper = graphs.GraphedStep(env, warmup=3) if graphed else env
        stepper.reset()
        for t in (range(8) if graphed else [0, 0, 0] + list(range(8))):
            actions = torch.as_tensor(np.random.RandomState(100 + t).choice([1, 3, 5], (16, 1)), device='cuda')
            world = stepper.step(arrdict.arrdict(actions=actions))
            logs.append([_np(x).copy() for x in (world.obs.rgb, world.obs.d, world.obs.goal, world.reward, world.reset, env.core.agents.positions,
                                                  env.walkers.positions, env.walkers.store.velocities, env.walkers.goal, env.frame.items)])
    eager, graphed = logs[3:11], logs[11:]
    assert [x.shape for x in graphed[0][:2]] == [(16, 1, 3, 1, 64), (16, 1, 1, 1, 64)] and graphed[0][6].shape == (16, 12, 2)
    assert all(np.array_equal(bits(g), bits(e)) if g.dtype == np.float32 else np.array_equal(g, e) for gs, es in zip(graphed, eager) for g, e in zip(gs, es))
    assert np.isfinite(graphed[-1][6]).all() and np.abs(graphed[-1][6] - graphed[0][6]).max() > .1 and any((step[9] >= 0).any() for step in graphed)


def test_overlay_items_shows_a_walker_that_stands_in_front_of_an_agent():
    from megastep_amd import cuda
    c, store = _core(plans(2), 1, 64), cuda.walkers(2, 3)
    heading = torch.deg2rad(c.agents.angles[:, 0])
    store.positions[:, 1] = c.agents.positions[:, 0] + .3*torch.stack([torch.cos(heading), torch.sin(heading)], -1)
    walked = cuda.walk(c.scenery, c.agents, store, torch.full((2, 3, 2), NAN, device='cuda'), agents_push=False)
    assert _np(walked.close).tolist() == [[1], [1]] and (_np(walked.blocked)[:, [0, 2]] == 4).all() and (_np(walked.blocked)[:, 1] < 4).all()
    frame = cuda.render(c.scenery, c.agents)
    open_ahead = _np(frame.distances[:, 0, 28:36].min(-1).values > .6)          # (no wall between the agent and the walker)
    shown = _np(cuda.overlay_items(store, frame, agents=c.agents, radius=c.agent_radius).items)
    assert open_ahead.any() and (shown[open_ahead][:, 0, 28:36] == 1).all() and set(np.unique(shown)) <= {-1, 1}


def test_a_reset_env_alone_draws_its_destinations_fields_and_walkers_anew():
    """modules.Walkers on two envs, env 0 reset - eagerly, then in a replayed graph, which draws afresh: its goals and fields change and
    its walkers stand on their drawn cells; env 1 keeps goals and fields to the bit and its walkers walk on."""
    from megastep_amd import cuda, modules
    c = _core(plans(2), 1, 64)
    crowd = modules.Walkers(c, cuda.nav_grid(c.scenery, config=c.config), 6, n_goals=3)
    reset, (lo, mid, hi), step = torch.tensor([True, False], device='cuda'), (3*int(v) for v in crowd.grid.starts), 1.4/c.fps + 1e-4
    state = lambda: [_np(x).copy() for x in (crowd.fields.goals, crowd.fields.values, crowd.positions)]
    crowd()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        crowd(reset)
    for call in (lambda: crowd(reset), graph.replay):
        (goals, values, before), _, (goals1, values1, after) = state(), call(), state()
        assert np.array_equal(bits(goals[1]), bits(goals1[1])) and np.array_equal(bits(values[mid:hi]), bits(values1[mid:hi]))
        assert not np.array_equal(goals[0], goals1[0]) and not np.array_equal(bits(values[lo:mid]), bits(values1[lo:mid]))
        assert np.array_equal(bits(goals1[0]), bits(_np(crowd._cells.points)[0, 0])) and np.isfinite(after).all()
        assert (np.linalg.norm(after[1] - before[1], axis=-1) <= step).all() and (np.linalg.norm(after[0] - before[0], axis=-1) > step).any()
        assert (np.linalg.norm(after[0] - _np(crowd._spawns.points)[0, :, 0], axis=-1) <= step).all()
