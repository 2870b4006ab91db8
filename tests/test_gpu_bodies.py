"""Solid bodies on the GPU: physics_bodies_kernel against ms_host_bodies - the serial host statement of the same
per-pair functions, which tests/test_bodies_host.py holds to the rule over the oracle - as bits in positions, angles, velocities,
progress, blocker and contacts; at every stride count of the store, with and without a wall grid, at rest and moving; past the pair
list's capacity; next to the env's bookkeeping; and the call's plumbing."""
import numpy as np
import pytest
import torch

from tests import util
from tests.body_rule import F, KEYS, NAN, host_bodies
from tests.rollout_rule import world_of
from tests.test_gpu_physics_pack import _restore, _state
from tests.test_gpu_slide import TABLE, _extras, _host
from tests.test_gpu_wallgrid import _world

pytestmark = pytest.mark.gpu


def crowd(c, P, rng, spread=.6, speed=2.):
    """A store of P slots round the agents of c: env 0 full, env 1 EMPTY, the others a third absent; body k within `spread` of
    agent k % A, every seventh far off; velocities up to `speed`, every fifth a NaN."""
    from megastep_amd import cuda
    N, A = c.agents.angles.shape
    store = cuda.walkers(N, P)
    at = _host(c.agents.positions)[:, np.arange(P) % A] + rng.uniform(-spread, spread, (N, P, 2))
    at[:, ::7] += 30.
    at[rng.rand(N, P) < np.array([0., 1.] + [.34]*(N - 2))[:N, None]] = NAN
    v = rng.uniform(-speed, speed, (N, P, 2))
    v[:, ::5, 0] = NAN
    store.positions[:] = torch.as_tensor(at.astype(F), device='cuda')
    store.velocities[:] = torch.as_tensor(v.astype(F), device='cuda')
    return store


def both(c, store, moving, movement=None, respawn=None, lifespans=None, imu=None, what='', **call):
    """One step among the bodies on the device and by ms_host_bodies from the same state, equal as bits in every output; the agents
    are left where the step put them. Returns the Physics."""
    from megastep_amd import cuda
    extras, held = _extras(respawn, lifespans, imu)
    mv = None if movement is None else (_host(movement[0]), _host(movement[1]), movement[2])
    want = host_bodies(world_of(c), _host(store.positions), _host(store.velocities) if moving else None, mv, extras, c.agent_radius, c.fps)
    got = cuda.physics(c.scenery, c.agents, movement=movement, respawn=respawn, lifespans=lifespans, imu=imu,
                       bodies=dict(store=store, moving=moving), **call)
    torch.cuda.synchronize()
    a = c.agents
    for k, t in zip(KEYS, (a.positions, a.angles, a.velocity, a.angvelocity, got.progress, got.blocker, got.contacts)):
        util.assert_bits(t, want[k], what + k)
    for k in ([] if imu is None else ['imu']) + ([] if lifespans is None else ['lifespans', 'max_lifespans']):
        util.assert_bits(imu[0] if k == 'imu' else lifespans[k], held[k], what + k)
    return got


@pytest.mark.parametrize('grid', [True, False], ids=['wallgrid', 'nowallgrid'])
@pytest.mark.parametrize('P', [1, 64, 65, 1024])
@pytest.mark.parametrize('A', [1, 4])
def test_the_kernel_is_the_host_statement(A, P, grid):
    """One stride, a full stride, one beyond, the cap; env 1's store is empty beside full ones. Two steps each way: the second from
    the state the first left, an agent outside its grid and a NaN pose among them."""
    c, _ = _world(3, A, seed=4 + A, n_unique=3, grid=grid)
    rng = np.random.RandomState(P + A)
    store = crowd(c, P, rng)
    for moving in (False, True):
        for step in (0, 1):
            util.random_velocities(c, rng, speed=3.)
            if step:
                c.agents.positions[1, 0] = torch.tensor([-30., 2.], device='cuda')
                c.agents.positions[2, -1] = float('nan')
            p = both(c, store, moving, what=f'moving={moving} step {step}: ')
            assert (p.contacts[1] == 0).all() and (p.blocker[1] == -1).all()
            assert P == 1 or step or moving or ((p.blocker >= 0).any() and (p.contacts[0] > 0).any())


def test_more_pairs_than_the_list_holds():
    """Four agents inside a cluster of 512 bodies: every agent's contacts alone are most of a list's 320 pairs, so the list drains
    between the body chunks, and with the walls' pairs in it."""
    c, _ = _world(2, 4, seed=8, n_unique=2)
    rng = np.random.RandomState(1)
    c.agents.positions[:, 1:] = c.agents.positions[:, :1] + torch.as_tensor(rng.uniform(-.1, .1, (2, 3, 2)).astype(F), device='cuda')
    store = crowd(c, 512, rng, spread=.25)
    store.positions[1] = store.positions[0] - c.agents.positions[0, 0] + c.agents.positions[1, 0]       # (env 1 as full as env 0)
    util.random_velocities(c, rng, speed=3.)
    for moving in (False, True):
        p = both(c, store, moving)
        assert int(p.contacts[0].sum()) > 320 and int(p.contacts[1].sum()) > 320, p.contacts


def test_next_to_the_books_on_a_side_stream_and_in_a_graph():
    from megastep_amd import cuda
    N, A, S, dev = 3, 4, 3, 'cuda'
    c, _ = _world(N, A, seed=10, n_unique=3)
    rng = np.random.RandomState(11)
    store = crowd(c, 65, rng)
    util.random_velocities(c, rng, speed=2., spin=0.)
    c.agents.angles[:] = 90.                                             # (where the host's and the device's sine agree: exact)
    spots = c.agents.positions[:, :, None, :].repeat(1, 1, S, 1).contiguous() + torch.as_tensor(rng.uniform(-.02, .02, (N, A, S, 2)).astype(F), device=dev)
    respawn = dict(mask=torch.as_tensor(rng.rand(N, A) < .3, device=dev), choices=torch.as_tensor(rng.randint(-1, S + 1, (N, A)), device=dev),
                   positions=spots, angles=torch.full((N, A, S), 90., device=dev), after=False)
    lifespans = dict(lifespans=torch.as_tensor(rng.randint(0, 5, (N, A)).astype(np.int32), device=dev),
                     max_lifespans=torch.full((N, A), 4, dtype=torch.int32, device=dev),
                     fresh=torch.as_tensor(rng.randint(5, 9, (N, A)).astype(np.int32), device=dev))
    imu = (torch.zeros((N, A, 3), device=dev), 360., 10.)
    movement = (torch.as_tensor(rng.randint(-1, 6, (N, A)), device=dev), torch.tensor(TABLE[:5], dtype=torch.float32, device=dev), .875)
    p = both(c, store, True, movement=movement, respawn=respawn, lifespans=lifespans, imu=imu)
    assert respawn['mask'].any() and (p.progress < 1).any()
    respawn['after'] = True
    both(c, store, False, movement=movement, respawn=respawn, imu=imu, what='after: ')
    # a side stream, writing into an earlier call's Physics
    start = _state(c)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        again = both(c, store, True, movement=movement, what='side: ', out=p)
    assert again is p
    # a captured graph, replayed three times: each replay steps the agents on from where the last left them
    _restore(c, start)
    bodies = dict(store=store, moving=True)
    static = cuda.physics(c.scenery, c.agents, movement=movement, bodies=bodies)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cuda.physics(c.scenery, c.agents, movement=movement, bodies=bodies, out=static)
    _restore(c, start)
    replayed = []
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        replayed.append(_state(c) + [static.progress.clone(), static.blocker.clone(), static.contacts.clone()])
    _restore(c, start)
    for k in range(3):
        eager = cuda.physics(c.scenery, c.agents, movement=movement, bodies=bodies)
        for x, y in zip(replayed[k], _state(c) + [eager.progress, eager.blocker, eager.contacts]):
            util.assert_bits(x, y, f'replay {k}')


def test_the_default_path_and_the_refusals():
    """Without ``bodies`` the call is what it was - and what an empty store gives; bodies with slide, a store of another shape and
    65 agents are refused before anything is launched."""
    from megastep_amd import cuda
    c, _ = _world(3, 2, seed=14, n_unique=3)
    rng = np.random.RandomState(15)
    util.random_velocities(c, rng, speed=40.)                          # (fast enough to hit a wall)
    start = _state(c)
    plain = cuda.physics(c.scenery, c.agents)
    assert plain.blocker is None and plain.contacts is None
    after = _state(c)
    _restore(c, start)
    among = cuda.physics(c.scenery, c.agents, bodies=cuda.walkers(3, 16))
    for x, y in zip(_state(c) + [among.progress], after + [plain.progress]):
        util.assert_bits(x, y)
    assert (among.blocker == -1).all() and (among.contacts == 0).all() and (plain.progress < 1).any()
    for bad in (dict(bodies=cuda.walkers(3, 16), slide=True), dict(bodies=cuda.walkers(2, 16)), dict(bodies=dict(store=cuda.items(3, 16), moving=True)),
                dict(bodies=dict(store=cuda.walkers(3, 16), fast=True)), dict(bodies=cuda.walkers(3, 16), out=plain)):
        with pytest.raises(RuntimeError):
            cuda.physics(c.scenery, c.agents, **bad)
    many, _ = util.plan_world(1, 65, 64, 130., seed=3, toy='box')
    with pytest.raises(RuntimeError, match='64 agents'):
        cuda.physics(many.scenery, many.agents, bodies=cuda.walkers(1, 16))


def test_a_solid_crowd_steps_the_same_eagerly_and_as_a_graph():
    from megastep_amd import arrdict, graphs
    from megastep_amd.demo import Crowd
    from tests.test_navfield_host import plans
    assert Crowd(4, n_walkers=4, geometries=plans(4))._mover.bodies is None   # (the default builds what it built)
    logs = []
    for graphed in (False, True):
        torch.manual_seed(3); np.random.seed(3)
        env = Crowd(16, n_walkers=16, geometries=plans(16), max_lifespan=10**6, solid=True)
        assert env._mover.bodies is env.walkers.store
        stepper = graphs.GraphedStep(env, warmup=3) if graphed else env
        stepper.reset()
        log = []
        for t in (range(8) if graphed else [0, 0, 0] + list(range(8))):
            actions = torch.as_tensor(np.random.RandomState(100 + t).choice([1, 3, 5], (16, 1)), device='cuda')
            world = stepper.step(arrdict.arrdict(actions=actions))
            log.append([world.reward.clone(), world.reset.clone(), world.obs.goal.clone(), world.obs.rgb.clone(), world.obs.d.clone(),
                        env.core.agents.positions.clone(), env.walkers.positions.clone(), env.walkers.blocker.clone()])
        logs.append(log)
    eager, graphed = logs
    # (the graphed env's first step call is four steps - three of warm-up and the captured one: its k-th is the eager env's k + 3)
    for k in range(len(graphed)):
        for x, y in zip(graphed[k], eager[k + 3]):
            util.assert_bits(x, y, f'step {k}')
