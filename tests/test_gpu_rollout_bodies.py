"""Rollouts among bodies on the GPU: rollout_bodies_kernel against ms_host_rollouts_bodies as bits in all ten outputs, at
the edges of the store's strides and of a wave's candidates; against the step it forecasts; LookAhead and a solid Crowd on top of it."""
import functools

import numpy as np
import pytest
import torch

from tests import util
from tests.rollout_rule import world_of
from tests.test_gpu_bodies import _host, crowd
from tests.test_gpu_physics_pack import _restore, _state
from tests.test_gpu_rollouts import TABLE, _LookAhead, _plans
from tests.test_gpu_wallgrid import _world
from tests.test_navfield_host import plans
from tests.test_rollout_bodies_host import KEYS, host_rollouts_bodies

pytestmark = pytest.mark.gpu

STRAIGHT = TABLE[:5] + TABLE[7:]        # (no row turns: the agents head along angle 0, where the host's sine and the device's agree)
N, KEEP = 3, .875


@functools.lru_cache(None)
def room(A, grid):
    """Three envs of A agents at angle 0 with velocities and no spin; never written to."""
    c, _ = _world(N, A, seed=4 + A, n_unique=3, grid=grid)
    util.random_velocities(c, np.random.RandomState(A), speed=2., spin=0.)
    c.agents.angles[:] = 0.
    return c


def both(c, store, moving, actions, table, what='', mask=None, out=None):
    """One call on the device and ms_host_rollouts_bodies env by env, equal as bits in every output. Returns the Rollouts."""
    from megastep_amd import cuda
    others = 'rest' if c.n_agents > 1 else None
    got = cuda.rollouts(c.scenery, c.agents, actions, table, keep=KEEP, others=others, trail=True, mask=mask, out=out,
                        bodies=dict(store=store, moving=moving))
    if out is None:
        want = host_rollouts_bodies(world_of(c), _host(actions), _host(table), KEEP, others, _host(store.positions),
                                    _host(store.velocities) if moving else None, c.agent_radius, c.fps, mask=None if mask is None else _host(mask))
        for k in KEYS:
            util.assert_bits(getattr(got, k), want[k], what + k)
    return got


@pytest.mark.parametrize('grid', [True, False], ids=['wallgrid', 'nowallgrid'])
@pytest.mark.parametrize('A', [1, 3])
@pytest.mark.parametrize('K', [1, 64, 65])
@pytest.mark.parametrize('P', [1, 64, 65, 1024])
def test_the_kernel_is_the_host_statement(P, K, A, grid):
    """test_gpu_bodies' crowd of P slots round the agents - env 0 full, env 1 empty, env 2 a third absent - at rest (the box) and moving."""
    c = room(A, grid)
    store = crowd(c, P, np.random.RandomState(P + A))
    table = torch.tensor(STRAIGHT, dtype=torch.float32, device='cuda')
    for moving in (False, True):
        for H in (1, 8):
            r = both(c, store, moving, _plans(P + K + H, (N, A, K, H), len(STRAIGHT)), table, f'moving={moving} H={H}: ')
            assert (r.body_stops[1] == 0).all() and (r.first_blocker[1] == -1).all()
            assert ((r.body_stops > 0) == (r.first_blocker >= 0)).all() and (r.body_stops <= r.stops).all()
            assert min(P, K) < 64 or (r.body_stops > 0).any()


def test_under_a_mask_with_out_reused():
    c = room(3, True)
    store = crowd(c, 65, np.random.RandomState(6))
    table = torch.tensor(STRAIGHT, dtype=torch.float32, device='cuda')
    actions = _plans(5, (N, 3, 20, 4), len(STRAIGHT))
    mask = torch.tensor([[1, 0, 1], [0, 0, 0], [0, 1, 0]], dtype=torch.bool, device='cuda')
    some = both(c, store, True, actions, table, mask=mask)                 # (the host leaves the rows the mask leaves out as fresh buffers are)
    whole = both(c, store, False, actions, table)
    held = {k: getattr(whole, k).clone() for k in KEYS}
    again = both(c, store, True, actions, table, mask=mask, out=whole)
    assert again is whole
    for k in KEYS:
        util.assert_bits(getattr(whole, k)[mask], getattr(some, k)[mask], k)
        util.assert_bits(getattr(whole, k)[~mask], held[k][~mask], k)


@pytest.mark.parametrize('moving', [False, True], ids=['rest', 'moving'])
def test_the_trail_is_the_step_among_bodies_chained_on_the_device(moving):
    """K = 3, H = 4, turning rows and all: every plan's trail against H cuda.physics(bodies=) steps, the store moved on between them."""
    from megastep_amd import cuda
    K, H = 3, 4
    c, _ = _world(N, 1, seed=9, n_unique=3)
    rng = np.random.RandomState(10)
    util.random_velocities(c, rng, speed=2.)
    store = crowd(c, 20, rng)
    table = torch.tensor(TABLE[:7], dtype=torch.float32, device='cuda')
    actions = _plans(11, (N, 1, K, H), 7)
    rolled = cuda.rollouts(c.scenery, c.agents, actions, table, keep=KEEP, trail=True, bodies=dict(store=store, moving=moving))
    start, q0 = _state(c), store.positions.clone()
    u = store.velocities/torch.full_like(store.velocities, c.fps)        # (a tensor's quotient: a scalar's is a product by 1/fps)
    u = torch.where(torch.isfinite(store.velocities).all(-1, keepdim=True), u, torch.zeros_like(u))
    for k in range(K):
        _restore(c, start)
        store.positions[:] = q0
        for h in range(H):
            cuda.physics(c.scenery, c.agents, movement=(actions[:, :, k, h].contiguous(), table, KEEP), bodies=dict(store=store, moving=moving))
            util.assert_bits(rolled.trail[:, 0, k, h], c.agents.positions[:, 0], f'plan {k} step {h}')
            if moving:
                store.positions[:] = store.positions + u
    assert (rolled.body_stops > 0).any() and (rolled.body_stops == 0).any()


def _crowd():
    from megastep_amd.demo import Crowd
    torch.manual_seed(3); np.random.seed(3)
    return Crowd(16, n_walkers=16, geometries=plans(16), max_lifespan=10**6, solid=True)


def test_lookahead_among_bodies_replays_as_a_graph():
    from megastep_amd import arrdict, modules
    env = _crowd()
    env.reset()
    among = dict(store=env.walkers.store, moving=True)
    look = modules.LookAhead(env.core, env._goals, env._mover, bodies=among, body_cost=.75)    # (a quarter above stop_cost)
    look()                                                               # (the buffers are made outside the graph)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        look()
    stopped = 0
    for t in range(4):
        env.step(arrdict.arrdict(actions=torch.full((16, 1), 1 + 2*(t % 2), dtype=torch.long, device='cuda')))
        graph.replay()
        torch.cuda.synchronize()
        eager = env._mover.rollouts(look.plans, bodies=among)
        for k in KEYS[:7] + KEYS[8:]:
            util.assert_bits(getattr(look.rolled, k), getattr(eager, k), f'replay {t}: {k}')
        values = env._goals.fields.at(eager.positions.view(16, 49, 2), goal=look._agent).view(16, 1, 49) + .25*eager.body_stops.float()
        util.assert_bits(look.values, values, f'replay {t}: values')
        stopped += int((eager.body_stops > 0).sum())
    assert stopped > 0


def test_a_solid_crowd_steps_under_the_lookahead_expert_eagerly_and_as_a_graph():
    from megastep_amd import arrdict, graphs
    logs = []
    for graphed in (False, True):
        env = _crowd()
        stepper = graphs.GraphedStep(_LookAhead(env), warmup=3) if graphed else _LookAhead(env)
        stepper.reset()
        env.expert('lookahead')                                          # (the expert and its buffers are made outside the graph)
        assert env._lookahead.bodies == dict(store=env.walkers.store, moving=True) and env._lookahead.rolled.body_stops is not None
        nothing = arrdict.arrdict(actions=torch.zeros((16, 1), dtype=torch.long, device='cuda'))
        log = []
        for _ in range(8 if graphed else 11):
            world = stepper.step(nothing)
            log.append([world.reward.clone(), world.reset.clone(), world.obs.goal.clone(), env.core.agents.positions.clone(),
                        env.walkers.positions.clone(), env._lookahead.rolled.body_stops.clone()])
        logs.append(log)
    eager, graphed = logs
    for k in range(len(graphed)):
        for x, y in zip(graphed[k], eager[k + 3]):
            util.assert_bits(x, y, f'step {k}')                          # (the graphed env's first step call is its warm-up's three and one)
    assert not torch.equal(eager[0][3], eager[-1][3])
