"""cuda.rollouts on the GPU: the kernel against the step it chains - for every candidate the agents restored and cuda.physics
called once per step of the plan - as bits in every output; with and without a wall grid; at every candidate count round a
wave's 64 lanes; the call's plumbing (mask, out, shared plans, a side stream, a captured graph); against the rule over the CPU
oracle; and LookAhead and PointGoal's 'lookahead' expert on top of it."""
import numpy as np
import pytest
import torch

from tests import util
from tests.rollout_rule import FIELDS, rollout_rule, world_of
from tests.test_navfield_host import plans
from tests.test_gpu_wallgrid import _world
from tests.test_gpu_physics_pack import _restore, _state

pytestmark = pytest.mark.gpu

# row 0 is the no-op; rows 1-6 the movement modules' actions at 3 m/s and 90 degrees a step; row 7 takes 2 m a step - farther than
# the wall grid's lists reach (1.3 m); row 8 crawls at 6e-7 m a step, where project()'s "+ 1e-6" stretches the reach to metres
TABLE = [[0, 0, 0], [0, 3, 0], [0, -3, 0], [3, 0, 0], [-3, 0, 0], [0, 0, 90], [0, 0, -90], [0, 20, 0], [0, 6e-6, 0]]


def _table():
    return torch.tensor(TABLE, dtype=torch.float32, device='cuda')


def _plans(seed, shape, n_actions=9):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, n_actions, shape, generator=g).cuda()


def _odd_poses(c, rng, nan=True):
    """Velocities for everyone; env 1's first agent outside its grid, env 2's faster than the lists reach, env 3's crawling, and
    (``nan``) env 4's at a NaN pose."""
    util.random_velocities(c, rng, speed=2.)
    pos, vel = c.agents.positions.clone(), c.agents.velocity.clone()
    pos[1, 0] = torch.tensor([-30., 2.])
    vel[2, 0] *= 20.
    vel[3, 0] *= 1e-7
    if nan:
        pos[4, 0] = float('nan')
    c.agents.positions[:] = pos
    c.agents.velocity[:] = vel


def stepped(c, actions, table, keep, others=None):
    """The reference: for every agent a and candidate k the agents restored, then H calls of cuda.physics under the movement
    prologue - with ``others='rest'`` everyone but a at zero velocity and the no-op action (row 0), else one agent per env.
    Returns the eight outputs as tensors."""
    from megastep_amd import cuda
    N, A = c.agents.angles.shape
    K, H = actions.shape[-2:]
    assert others == 'rest' or A == 1
    start = _state(c)
    dev = 'cuda'
    out = dict(positions=torch.empty((N, A, K, 2), device=dev), angles=torch.empty((N, A, K), device=dev),
               velocity=torch.empty((N, A, K, 2), device=dev), angvelocity=torch.empty((N, A, K), device=dev),
               progress=torch.empty((N, A, K), device=dev), stops=torch.empty((N, A, K), dtype=torch.int32, device=dev),
               first_stop=torch.empty((N, A, K), dtype=torch.int32, device=dev), trail=torch.empty((N, A, K, H, 2), device=dev))
    for a in range(A):
        only = torch.zeros((N, A), dtype=torch.bool, device=dev)
        only[:, a] = True
        for k in range(K):
            _restore(c, start)
            c.agents.velocity[:] = torch.where(only[..., None], start[2], torch.zeros_like(start[2]))
            c.agents.angvelocity[:] = torch.where(only, start[3], torch.zeros_like(start[3]))
            least = torch.ones(N, device=dev)
            stops = torch.zeros(N, dtype=torch.int32, device=dev)
            first = torch.full((N,), H, dtype=torch.int32, device=dev)
            for h in range(H):
                act = torch.where(only, actions[:, :, k, h], torch.zeros_like(actions[:, :, k, h])).contiguous()
                p = cuda.physics(c.scenery, c.agents, movement=(act, table, keep))
                x = p.progress[:, a]
                least = torch.minimum(least, x)
                stops += (x < 1).int()
                first = torch.where((x < 1) & (first == H), torch.full_like(first, h), first)
                out['trail'][:, a, k, h] = c.agents.positions[:, a]
            out['positions'][:, a, k], out['angles'][:, a, k] = c.agents.positions[:, a], c.agents.angles[:, a]
            out['velocity'][:, a, k], out['angvelocity'][:, a, k] = c.agents.velocity[:, a], c.agents.angvelocity[:, a]
            out['progress'][:, a, k], out['stops'][:, a, k], out['first_stop'][:, a, k] = least, stops, first
    _restore(c, start)
    return out


def _same(rolled, want, what=''):
    for k in FIELDS:
        got = getattr(rolled, k) if not isinstance(rolled, dict) else rolled[k]
        wanted = want[k] if isinstance(want, dict) else getattr(want, k)
        assert (got is None) == (wanted is None), k                      # (the trail: asked for by both, or by neither)
        if got is not None:
            util.assert_bits(got, wanted, f'{what}{k}')


@pytest.mark.parametrize('keep', [0., .875])
def test_one_agent_per_env_against_the_step_itself(keep):
    from megastep_amd import cuda
    N, K, H = 37, 49, 6
    c, _ = _world(N, 1, seed=4)
    _odd_poses(c, np.random.RandomState(5))
    actions, table = _plans(1, (N, 1, K, H)), _table()
    before = _state(c)
    rolled = cuda.rollouts(c.scenery, c.agents, actions, table, keep=keep, trail=True)
    for x, y in zip(_state(c), before):                                  # (the agents are not modified)
        util.assert_bits(x, y)
    want = stepped(c, actions, table, keep)
    _same(rolled, want)
    assert (rolled.stops > 0).any() and (rolled.stops == 0).any() and (rolled.first_stop < H).any()
    assert torch.isnan(rolled.positions[4]).all() and not torch.isnan(rolled.positions[:4]).any()


def test_four_agents_per_env_with_the_others_at_rest_against_the_step_itself():
    from megastep_amd import cuda
    N, A, K, H = 9, 4, 16, 4
    c, _ = _world(N, A, seed=6)
    _odd_poses(c, np.random.RandomState(7), nan=False)
    pos = c.agents.positions.clone()
    pos[5, 1] = pos[5, 0] + torch.tensor([.25, 0.], device='cuda')       # a pair a step apart
    c.agents.positions[:] = pos
    actions, table = _plans(2, (N, A, K, H)), _table()
    rolled = cuda.rollouts(c.scenery, c.agents, actions, table, keep=.875, others='rest', trail=True)
    want = stepped(c, actions, table, .875, others='rest')
    _same(rolled, want)
    assert (rolled.stops > 0).any() and (rolled.stops == 0).any()
    absent = cuda.rollouts(c.scenery, c.agents, actions, table, keep=.875, trail=True)
    assert not torch.equal(absent.stops[5], rolled.stops[5])             # (the pair: obstacles to each other only when asked)


@pytest.mark.parametrize('n_agents,others', [(1, None), (3, 'rest')])
def test_with_and_without_a_wall_grid(n_agents, others):
    from megastep_amd import cuda
    N, K, H = 24, 70, 5
    worlds = [_world(N, n_agents, seed=3, n_unique=6, grid=g)[0] for g in (True, False)]
    assert worlds[0].scenery._wg is not None and worlds[1].scenery._wg is None
    actions, table = _plans(3, (N, n_agents, K, H)), _table()
    got = []
    for c in worlds:
        _odd_poses(c, np.random.RandomState(8))
        got.append(cuda.rollouts(c.scenery, c.agents, actions, table, keep=.875, others=others, trail=True))
    _same(got[0], got[1])
    assert (got[0].stops > 0).any() and (got[0].stops == 0).any()


@pytest.fixture
def scheme():
    from megastep_amd import _lib
    h = _lib.lib()
    yield h.ms_debug_rollout_scheme
    h.ms_debug_rollout_scheme(-1)


@pytest.mark.parametrize('n_agents,others,grid', [(1, None, True), (3, 'rest', True), (2, 'rest', False)])
def test_either_scheme_leaves_the_same_bits(scheme, n_agents, others, grid):
    """A lane a candidate (the library's) against a lane a wall, the candidates one after another (physics_kernel's scheme): with a
    wall grid and without, lists longer than a flush of the pair list leaves room for (the list's lengths window by window are
    counted in tests/test_gpu_step_edges.py::test_the_rollouts_list_at_its_capacity), K past one wave and not a multiple of it."""
    from megastep_amd import cuda
    N, K, H = 11, 100, 5
    c, _ = _world(N, n_agents, seed=13, n_unique=5, grid=grid)
    _odd_poses(c, np.random.RandomState(14))
    actions, table = _plans(7, (N, n_agents, K, H)), _table()
    mask = torch.ones((N, n_agents), dtype=torch.bool, device='cuda')
    mask[6] = False
    got = []
    for which in (0, 1, -1):
        assert scheme(which) == 0
        got.append(cuda.rollouts(c.scenery, c.agents, actions, table, keep=.875, others=others, trail=True, mask=mask))
    _same(got[1], got[0])
    _same(got[2], got[0])
    assert scheme(2) == -1 and scheme(-2) == -1
    assert (got[0].stops > 0).any() and (got[0].stops == 0).any() and torch.isnan(got[1].positions[6]).all()


def test_candidate_counts_round_a_wave():
    from megastep_amd import cuda
    N, A, H = 5, 2, 3
    c, _ = _world(N, A, seed=9)
    _odd_poses(c, np.random.RandomState(10))
    actions, table = _plans(4, (N, A, 256, H)), _table()
    whole = cuda.rollouts(c.scenery, c.agents, actions, table, keep=.875, others='rest', trail=True)
    for K in (1, 24, 25, 63, 64, 65, 128, 256):                         # (24 | 25: where the library changes its scheme)
        part = cuda.rollouts(c.scenery, c.agents, actions[:, :, :K].contiguous(), table, keep=.875, others='rest', trail=True)
        for k in FIELDS:
            util.assert_bits(getattr(part, k), getattr(whole, k)[:, :, :K].contiguous(), f'K = {K}: {k}')
        if K == 64:
            _same(part, stepped(c, actions[:, :, :K].contiguous(), table, .875, others='rest'), 'K = 64: ')
    assert (whole.stops > 0).any() and (whole.stops == 0).any()


def test_call_plumbing():
    from megastep_amd import cuda
    N, A, K, H = 6, 2, 20, 4
    c, _ = _world(N, A, seed=11)
    util.random_velocities(c, np.random.RandomState(12), speed=2.)
    shared, table = _plans(5, (K, H)), _table()
    before = _state(c)
    first = cuda.rollouts(c.scenery, c.agents, shared, table, keep=.875, others='rest', trail=True)
    for x, y in zip(_state(c), before):
        util.assert_bits(x, y, 'the agents after a call')
    # (K, H) plans against the expanded tensor
    expanded = cuda.rollouts(c.scenery, c.agents, shared[None, None].expand(N, A, K, H).contiguous(), table, keep=.875, others='rest', trail=True)
    _same(first, expanded)
    assert first.trail.shape == (N, A, K, H, 2) and cuda.rollouts(c.scenery, c.agents, shared, table).trail is None
    # mask: without out the others read as not rolled; with out they keep what it held
    mask = torch.zeros((N, A), dtype=torch.bool, device='cuda')
    mask[::2, 0] = True; mask[1, 1] = True
    some = cuda.rollouts(c.scenery, c.agents, shared, table, keep=.875, others='rest', trail=True, mask=mask)
    for k in FIELDS:
        util.assert_bits(getattr(some, k)[mask], getattr(first, k)[mask], k)
    assert torch.isnan(some.positions[~mask]).all() and torch.isnan(some.trail[~mask]).all() and (some.progress[~mask] == 1).all()
    assert (some.stops[~mask] == 0).all() and (some.first_stop[~mask] == H).all()
    # out=: rewritten in place, the rows the mask leaves out untouched
    held = {k: getattr(first, k).clone() for k in FIELDS}
    ptrs = [getattr(first, k).data_ptr() for k in FIELDS]
    util.random_velocities(c, np.random.RandomState(13), speed=2.)
    again = cuda.rollouts(c.scenery, c.agents, shared, table, keep=.875, others='rest', trail=True, mask=mask, out=first)
    fresh = cuda.rollouts(c.scenery, c.agents, shared, table, keep=.875, others='rest', trail=True)
    assert again is first and ptrs == [getattr(first, k).data_ptr() for k in FIELDS]
    for k in FIELDS:
        util.assert_bits(getattr(first, k)[mask], getattr(fresh, k)[mask], k)
        util.assert_bits(getattr(first, k)[~mask], held[k][~mask], k)
    with pytest.raises(RuntimeError, match='out'):
        cuda.rollouts(c.scenery, c.agents, shared[:5].contiguous(), table, keep=.875, others='rest', trail=True, out=first)
    # a side stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        aside = cuda.rollouts(c.scenery, c.agents, shared, table, keep=.875, others='rest', trail=True)
    side.synchronize()
    _same(aside, fresh)
    # a captured graph, replayed after the agents moved
    static = cuda.rollouts(c.scenery, c.agents, shared, table, keep=.875, others='rest', trail=True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cuda.rollouts(c.scenery, c.agents, shared, table, keep=.875, others='rest', trail=True, out=static)
    util.random_velocities(c, np.random.RandomState(14), speed=2.)
    c.agents.positions[:] = c.agents.positions + .05
    graph.replay()
    torch.cuda.synchronize()
    _same(static, cuda.rollouts(c.scenery, c.agents, shared, table, keep=.875, others='rest', trail=True))
    assert not all(util.same_bits(getattr(static, k), getattr(fresh, k)).all() for k in ('positions', 'velocity'))


@pytest.mark.parametrize('others', [None, 'rest'])
def test_against_the_rule_over_the_oracle(oracle, others):
    """The kernel against tests/rollout_rule.py, whose collision and integration are the CPU oracle's. The rule's movement step is
    the host libm's sine and cosine, which need not round as the device's do: the agents here head along +y (angle 0, where both
    are exact) and the plans never turn, so every statement of the two sides is one the numerics contract covers."""
    from megastep_amd import cuda
    N, A, K, H = 3, 2, 12, 4
    c, _ = _world(N, A, seed=15)
    c.agents.angles[:] = 0.
    c.agents.positions[1, 1] = c.agents.positions[1, 0] + torch.tensor([0., .3], device='cuda')
    rng = np.random.RandomState(16)
    c.agents.velocity[:] = torch.as_tensor(rng.uniform(-2, 2, (N, A, 2)).astype(np.float32), device='cuda')
    table = _table()
    actions = _plans(6, (N, A, K, H), n_actions=5)
    actions[:, :, 0, 0] = 7                                              # (too fast for the lists)
    rolled = cuda.rollouts(c.scenery, c.agents, actions, table, keep=.875, others=others, trail=True)
    want = rollout_rule(world_of(c), actions.cpu().numpy(), table.cpu().numpy(), .875, others, c.agent_radius, c.fps)
    _same(rolled, want)
    assert (rolled.stops > 0).any() and (rolled.stops == 0).any()


class _LookAhead:
    """An env whose step is the look-ahead expert's: the decision handed in is ignored."""

    def __init__(self, env):
        self.env = env

    def __getattr__(self, name):
        return getattr(self.env, name)

    def step(self, decision):
        return self.env.step(self.env.expert('lookahead'))


def test_lookahead_takes_what_its_rule_says_of_its_own_rollouts():
    from megastep_amd import cuda, modules
    from megastep_amd.demo import PointGoal
    torch.manual_seed(3); np.random.seed(3)
    env = PointGoal(16, geometries=plans(16), max_lifespan=10**6)
    env.reset()
    follow = env.expert()                                                # (what it returned before: the follower's decision, key for key)
    assert list(follow.keys()) == ['actions'] and follow.actions.shape == (16, 1) and follow.actions.dtype == torch.int64
    assert torch.equal(follow.actions, modules.PathFollower(env.core, env._goals, cone=15.)().actions)
    look = modules.LookAhead(env.core, env._goals, env._mover)
    assert look.plans.shape == (49, 8) and torch.equal(look.plans, cuda.plans(7, 8, 2, device='cuda'))
    chosen = 0
    for _ in range(6):
        decision = look()
        assert decision.actions.shape == (16, 1) and decision.actions.dtype == torch.int64
        action, none = modules.LookAhead.choose(look.values, look.rolled.stops, look.plans, look.stop_cost)
        assert torch.equal(look.values, env._goals.fields.at(look.rolled.positions.view(16, 49, 2), goal=look._agent).view(16, 1, 49))
        assert torch.equal(decision.actions[~none], action[~none])
        chosen += int((~none).sum())
        _same(look.rolled, env._mover.rollouts(look.plans))
        env.step(decision)
    assert chosen > 48
    with pytest.raises(RuntimeError, match='kind'):
        env.expert('fly')


def test_pointgoal_steps_under_the_lookahead_expert_eagerly_and_as_a_graph():
    from megastep_amd import arrdict, graphs
    from megastep_amd.demo import PointGoal
    logs = []
    for graphed in (False, True):
        torch.manual_seed(3); np.random.seed(3)
        env = PointGoal(16, geometries=plans(16), max_lifespan=10**6)
        stepper = graphs.GraphedStep(_LookAhead(env), warmup=3) if graphed else _LookAhead(env)
        stepper.reset()
        env.expert('lookahead')                                          # (the expert and its buffers are made outside the graph)
        nothing = arrdict.arrdict(actions=torch.zeros((16, 1), dtype=torch.long, device='cuda'))
        log = []
        for _ in range(20 if graphed else 23):
            world = stepper.step(nothing)
            log.append([world.reward.clone(), world.reset.clone(), world.obs.goal.clone(), env.core.agents.positions.clone(),
                        env.core.agents.angles.clone(), env.core.agents.velocity.clone()])
        logs.append(log)
    eager, graphed = logs
    # the graphed env's first step call is four steps (three of warm-up and the captured one): its k-th is the eager env's k + 3
    for k in range(len(graphed)):
        for x, y in zip(graphed[k], eager[k + 3]):
            util.assert_bits(x, y, f'step {k}')
    assert not torch.equal(eager[0][3], eager[-1][3])
