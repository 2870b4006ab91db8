"""Projectiles on the GPU: projectile_kernel held to EQUALITY with its host instantiation - which the CPU suite holds to fly_rule - in
the whole store and every record, floats by their bits; then what is built on it (modules.Projectiles, demo.Dodge, the overlay)."""
import numpy as np
import pytest
import torch

from tests import projectile_rule as pr
from tests.projectile_rule import KEYS, NAN
from tests.test_navfield_host import plans
from tests.test_gpu_navseen import _core, _np
from tests.test_gpu_navview import _walls

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device='cuda')


def _world(geoms, A, S, seed, speed=8., lo=None, hi=None):
    """The plans as a scenery of A agents posed at random in their bounding boxes, pr.random_store() in the same boxes and on the device."""
    from megastep_amd import core, cuda, scene
    sc = scene.scenery(geoms, A, device='cuda', bake=False)
    agents, walls, N = core._init_agents(len(geoms), A, 'cuda'), _walls(sc), len(geoms)
    agents._config = cuda.config(core.AGENT_RADIUS, 64, 130, 10)
    lo, hi = lo or [w.reshape(-1, 2).min(0) for w in walls], hi or [w.reshape(-1, 2).max(0) for w in walls]
    rng = np.random.RandomState(seed)
    agents.positions.copy_(_dev(np.stack([rng.uniform(lo[n], hi[n], (A, 2)) for n in range(N)]).astype(np.float32)))
    agents.angles.copy_(_dev(rng.uniform(-180, 180, (N, A)).astype(np.float32)))
    store, dev = pr.random_store(N, A, S, lo, hi, seed, speed), cuda.projectiles(N, A, S)
    return sc, agents, walls, store, dev


def _tick(sc, agents, walls, store, dev, load=True, fly=None, **kw):
    """One tick on the device - cuda.fly, or `fly()` - and by the host statement from the numpy `store`, compared: the store after it."""
    from megastep_amd import cuda
    for k in pr.STORE if load else ():
        getattr(dev, k).copy_(_dev(store[k]))
    flown = fly() if fly else cuda.fly(sc, agents, dev, **{k: _dev(v) if isinstance(v, np.ndarray) else v for k, v in kw.items()})
    torch.cuda.synchronize()
    want = pr.host_fly(walls, _np(sc.model).reshape(-1, 4), _np(agents.positions), _np(agents.angles), store, **kw)
    pr.same({k: _np(getattr(dev if k in pr.STORE else flown, k)) for k in KEYS}, want, KEYS)
    return {k: want[k] for k in pr.STORE}, want, flown


@pytest.mark.parametrize('N', [1, 3])
@pytest.mark.parametrize('A,S', [(1, 1), (4, 16), (5, 13), (16, 16), (43, 6), (64, 16)])
def test_the_kernel_is_its_host_statement_round_a_wave_and_a_chunk(A, S, N):
    """P = 1, 64, 65, 256, 258 (257 is a prime) and 1024, two ticks; of three envs the middle one has nothing in flight, nobody firing."""
    sc, agents, walls, store, dev = _world((plans(3) + plans(3, oblique=True))[1:1 + N], A, S, A*S)
    fire = (np.random.RandomState(A).rand(N, A) < .5).astype(np.uint8)
    if N == 3:
        store['positions'][1], fire[1] = NAN, 0
    for _ in range(2):
        store, want, _ = _tick(sc, agents, walls, store, dev, fire=fire, bounces=3, life=3, restitution=.8)
    assert (want['ended'] < 4).any() and (N == 1 or (want['ended'][1] == 4).all())


def test_an_env_whose_kept_rows_overflow_the_list_walks_global_memory():
    """700 short walls in the room, the shots in a corner of it: at 300 m/s the union box covers the plan, at 2 m/s it does not."""
    rng = np.random.RandomState(5)
    a = rng.uniform((.2, .2), (7.8, 3.8), (700, 2))
    room = np.concatenate([pr.ROOM, np.concatenate([a, a + rng.uniform(-.1, .1, (700, 2))], 1).astype(np.float32)])
    for speed, over in ((300., True), (2., False)):
        sc, agents, walls, store, dev = _world([dict(walls=room.reshape(-1, 2, 2), lights=np.array([[1., 1.]]))], 2, 16, 3, speed, [(.5, .5)], [(2.5, 1.5)])
        flying, w = np.isfinite(store['positions'][0]).all(-1), walls[0]
        r = (np.abs(store['velocities'][0]/np.float32(10)).sum(-1)*1.01 + 1e-3)[:, None]
        lo, hi = (store['positions'][0] - r)[flying].min(0), (store['positions'][0] + r)[flying].max(0)
        listed = ((w[:, 0::2].min(1) <= hi[0]) & (w[:, 0::2].max(1) >= lo[0]) & (w[:, 1::2].min(1) <= hi[1]) & (w[:, 1::2].max(1) >= lo[1])).sum()
        assert (listed > 512) == over and listed > 20
        after, want, _ = _tick(sc, agents, walls, store, dev)
        assert not over or (want['ended'] == 2).any() or (after['bounces'] != store['bounces']).any()


@pytest.mark.parametrize('first', [0, 3])
def test_sixteen_ticks_in_a_row_with_fire_every_fourth_then_three_replays_of_a_graph(first):
    """Two plans a case, the store compared after every tick; `out=` on a side stream; then three replays, each a later tick."""
    from megastep_amd import cuda
    sc, agents, walls, store, dev = _world((plans(3) + plans(3, oblique=True))[first:first + 2], 3, 8, first)
    kw = dict(speed=6., muzzle=.3, life=7, bounces=2, restitution=.9)
    side, fire, flown = torch.cuda.Stream(), torch.zeros((2, 3), dtype=torch.uint8, device='cuda'), None

    def eager():
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            out = cuda.fly(sc, agents, dev, fire=fire, out=flown, **kw)
        assert flown is None or out is flown
        return out

    for t in range(16):
        fire.fill_(t % 4 == 0)
        store, _, flown = _tick(sc, agents, walls, store, dev, load=t == 0, fly=eager, fire=_np(fire), **kw)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cuda.fly(sc, agents, dev, fire=fire, out=flown, **kw)
    for t in range(3):
        fire.fill_(t == 1)
        store, _, _ = _tick(sc, agents, walls, store, dev, load=t == 0, fly=lambda: graph.replay() or flown, fire=_np(fire), **kw)
    assert np.isfinite(store['positions']).all(-1).any()


def test_dodge_as_one_hip_graph_equals_the_eager_env_key_for_key():
    from megastep_amd import arrdict, graphs
    from megastep_amd.demo import Dodge
    logs = []
    for graphed in (False, True):
        torch.manual_seed(3); np.random.seed(3)
        env = Dodge(16, geometries=plans(16), max_lifespan=10**6, life=12, bounces=1)
        stepper = graphs.GraphedStep(env, warmup=3) if graphed else env
        stepper.reset()
        for t in (range(8) if graphed else [0, 0, 0] + list(range(8))):
            actions = torch.as_tensor(np.random.RandomState(100 + t).choice([1, 5, 7, 7], (16, 2)), device='cuda')
            world = stepper.step(arrdict.arrdict(actions=actions))
            logs.append([_np(x).copy() for x in (world.obs.rgb, world.obs.d, world.obs.percepts, world.reward, world.reset,
                                                  env.core.agents.positions, env.projectiles.positions, env.frame.items)])
    eager, graphed = logs[3:11], logs[11:]
    assert [x.shape for x in graphed[0][:3]] == [(16, 2, 3, 1, 64), (16, 2, 1, 1, 64), (16, 2, 4, 4)] and graphed[0][7].shape == (16, 2, 256)
    assert all(np.array_equal(pr.ir.bits(g), pr.ir.bits(e)) for gs, es in zip(graphed, eager) for g, e in zip(gs, es))
    assert any(np.isfinite(step[6]).any() for step in graphed) and any((step[7] >= 0).any() for step in graphed)


def test_overlay_items_shows_a_projectile_in_flight():
    from megastep_amd import cuda, modules
    c = _core(plans(2), 2, 64)
    store = cuda.projectiles(2, 2, 2)
    cuda.fly(c.scenery, c.agents, store, fire=torch.ones((2, 2), dtype=torch.bool, device='cuda'), speed=.5, muzzle=.25)
    flying = _np(torch.isfinite(store.positions[:, ::2]).all(-1))              # (a shot fired into a wall at arm's length is gone)
    assert flying.any() and bool(torch.isnan(store.positions[:, 1::2]).all())
    shown = _np(cuda.overlay_items(store, cuda.render(c.scenery, c.agents), agents=c.agents, radius=.05).items)
    assert all(2*a in shown[n, a] for n in range(2) for a in range(2) if flying[n, a])
    seen = _np(modules.Percepts(c, points=store.positions, fov=c.fov, k=2)())
    assert (seen[:, :, 0, 0][flying] == 1).all()
