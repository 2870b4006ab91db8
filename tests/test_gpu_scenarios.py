"""cuda.scenarios and the focal mode of cuda.rollouts on the GPU: the kernel against the step it chains - for every scenario the
agents restored and cuda.physics called once per step, everybody on its own action - as bits in every output, at the shapes
where the lane mapping can go wrong (G = 64 // A scenarios a wave, idle lanes, S across a wave); one agent an env against
cuda.rollouts; with and without a wall grid; a scenario's result whatever S is; the focal mode against the step and against
the joint call; the call's plumbing; and LookAhead(others='repeat') and PointGoal's 'anticipate' expert on top of it."""
import numpy as np
import pytest
import torch

from tests import util
from tests.rollout_rule import FIELDS
from tests.test_navfield_host import plans
from tests.test_gpu_wallgrid import _world
from tests.test_gpu_physics_pack import _restore, _state
from tests.test_gpu_rollouts import TABLE, _odd_poses, _plans, _same, _table

pytestmark = pytest.mark.gpu


def _odd(c, rng):
    """test_gpu_rollouts._odd_poses, which needs five envs; in fewer, the oddities that have an env to be in."""
    N = c.agents.angles.shape[0]
    if N >= 5:
        return _odd_poses(c, rng)
    util.random_velocities(c, rng, speed=2.)
    pos, vel = c.agents.positions.clone(), c.agents.velocity.clone()
    pos[0, 0] = float('nan')
    pos[1, 0] = torch.tensor([-30., 2.])
    vel[1, 1] *= 20.
    vel[N - 1, 1] *= 1e-7
    c.agents.positions[:] = pos
    c.agents.velocity[:] = vel


def _pair(c, n, a, b, gap=.25):
    """Agent b of env n a step away from agent a."""
    pos = c.agents.positions.clone()
    pos[n, b] = pos[n, a] + torch.tensor([gap, 0.], device='cuda')
    c.agents.positions[:] = pos


def _books(N, rows, H):
    dev = 'cuda'
    return dict(positions=torch.empty((N, *rows, 2), device=dev), angles=torch.empty((N, *rows), device=dev),
                velocity=torch.empty((N, *rows, 2), device=dev), angvelocity=torch.empty((N, *rows), device=dev),
                progress=torch.empty((N, *rows), device=dev), stops=torch.empty((N, *rows), dtype=torch.int32, device=dev),
                first_stop=torch.empty((N, *rows), dtype=torch.int32, device=dev), trail=torch.empty((N, *rows, H, 2), device=dev))


def _run(c, start, plan, table, keep):
    """The agents restored, then H calls of cuda.physics under plan (N, A, H): (state, least, stops, first, trail (N, A, H, 2))."""
    from megastep_amd import cuda
    N, A, H = plan.shape
    _restore(c, start)
    least = torch.ones((N, A), device='cuda')
    stops = torch.zeros((N, A), dtype=torch.int32, device='cuda')
    first = torch.full((N, A), H, dtype=torch.int32, device='cuda')
    trail = torch.empty((N, A, H, 2), device='cuda')
    for h in range(H):
        x = cuda.physics(c.scenery, c.agents, movement=(plan[:, :, h].contiguous(), table, keep)).progress
        least = torch.minimum(least, x)
        stops += (x < 1).int()
        first = torch.where((x < 1) & (first == H), torch.full_like(first, h), first)
        trail[:, :, h] = c.agents.positions
    return _state(c), least, stops, first, trail


def stepped(c, actions, table, keep):
    """The reference of the joint mode: for every scenario the agents restored, then H calls of cuda.physics with
    movement=(actions[:, s, :, h], table, keep). Returns the eight outputs (N, S, A, ..) as tensors."""
    N, S, A, H = actions.shape
    start = _state(c)
    out = _books(N, (S, A), H)
    for s in range(S):
        st, least, stops, first, trail = _run(c, start, actions[:, s], table, keep)
        out['positions'][:, s], out['angles'][:, s], out['velocity'][:, s], out['angvelocity'][:, s] = st
        out['progress'][:, s], out['stops'][:, s], out['first_stop'][:, s], out['trail'][:, s] = least, stops, first, trail
    _restore(c, start)
    return out


def expanded(plans_, base):
    """The joint tensor (N, A K, A, H) a focal call on plans (N, A, K, H) and base (N, A, H) means."""
    N, A, K, H = plans_.shape
    joint = base[:, None, None].expand(N, A, K, A, H).clone()
    for f in range(A):
        joint[:, f, :, f] = plans_[:, f]
    return joint.reshape(N, A*K, A, H)


@pytest.mark.parametrize('N, A, S, H, keep', [(9, 4, 20, 4, .875), (9, 4, 20, 4, 0.), (7, 3, 22, 3, .875), (5, 5, 13, 3, .875),
                                              (3, 33, 2, 2, .875), (2, 64, 2, 2, .875)])
def test_against_the_step_itself(N, A, S, H, keep):
    """G = 16 with S across a wave; G = 21, one idle lane, S = G + 1; G = 12, four idle lanes; G = 1 with 31 idle lanes; a full wave."""
    from megastep_amd import cuda
    c, _ = _world(N, A, seed=6)
    _odd(c, np.random.RandomState(7))
    _pair(c, N - 1, 0, 1)
    actions, table = _plans(2, (N, S, A, H)), _table()
    before = _state(c)
    got = cuda.scenarios(c.scenery, c.agents, actions, table, keep=keep, trail=True)
    for x, y in zip(_state(c), before):                                  # (the agents are not modified)
        util.assert_bits(x, y)
    _same(got, stepped(c, actions, table, keep))
    if (N, A) == (9, 4):
        # who stopped whom: alone in its env an agent walks the same way until something stops it - a first stop that comes
        # earlier among the others is an agent's doing, one at the same step a wall's
        alone = cuda.rollouts(c.scenery, c.agents, actions.transpose(1, 2).contiguous(), table, keep=keep).first_stop.transpose(1, 2)
        assert (got.first_stop < alone).any(), 'nobody was stopped by an agent'
        assert ((got.first_stop == alone) & (alone < H)).any(), 'nobody was stopped by a wall'
        assert (got.stops == 0).any(), 'everybody was stopped'


def test_one_agent_an_env_is_the_rollouts_call():
    from megastep_amd import cuda
    N, K, H = 37, 49, 6
    c, _ = _world(N, 1, seed=4)
    _odd_poses(c, np.random.RandomState(5))
    actions, table = _plans(1, (N, K, 1, H)), _table()
    got = cuda.scenarios(c.scenery, c.agents, actions, table, keep=.875, trail=True)
    want = cuda.rollouts(c.scenery, c.agents, actions.transpose(1, 2).contiguous(), table, keep=.875, trail=True)
    for k in FIELDS:
        util.assert_bits(getattr(got, k).transpose(1, 2).contiguous(), getattr(want, k), k)
    assert (got.stops > 0).any() and (got.stops == 0).any()


def test_with_and_without_a_wall_grid():
    from megastep_amd import cuda
    N, A, S, H = 24, 3, 30, 5
    worlds = [_world(N, A, seed=3, n_unique=6, grid=g)[0] for g in (True, False)]
    assert worlds[0].scenery._wg is not None and worlds[1].scenery._wg is None
    actions, table = _plans(3, (N, S, A, H)), _table()
    got = []
    for c in worlds:
        _odd_poses(c, np.random.RandomState(8))
        _pair(c, 7, 0, 1)
        got.append(cuda.scenarios(c.scenery, c.agents, actions, table, keep=.875, trail=True))
    _same(got[0], got[1])
    assert (got[0].stops > 0).any() and (got[0].stops == 0).any()


def test_a_scenario_does_not_depend_on_how_many_there_are():
    from megastep_amd import cuda
    N, A, H = 5, 4, 2
    c, _ = _world(N, A, seed=9)
    _odd_poses(c, np.random.RandomState(10))
    _pair(c, 2, 1, 2)
    actions, table = _plans(4, (N, 256, A, H)), _table()
    whole = cuda.scenarios(c.scenery, c.agents, actions, table, keep=.875, trail=True)
    for S in (1, 16, 17, 255, 256):                                      # (G = 16)
        part = cuda.scenarios(c.scenery, c.agents, actions[:, :S].contiguous(), table, keep=.875, trail=True)
        for k in FIELDS:
            util.assert_bits(getattr(part, k), getattr(whole, k)[:, :S].contiguous(), f'S = {S}: {k}')
    assert (whole.stops > 0).any() and (whole.stops == 0).any()


def test_the_focal_mode_against_the_step_itself():
    from megastep_amd import cuda
    N, A, K, H = 5, 4, 7, 4
    c, _ = _world(N, A, seed=12)
    _odd_poses(c, np.random.RandomState(13))
    _pair(c, 3, 0, 1)
    plans_, base, table = _plans(5, (N, A, K, H)), _plans(6, (N, A, H)), _table()
    got = cuda.rollouts(c.scenery, c.agents, plans_, table, keep=.875, others=base, trail=True)
    start = _state(c)
    want = _books(N, (A, K), H)
    for f in range(A):
        for k in range(K):
            plan = base.clone()
            plan[:, f] = plans_[:, f, k]
            st, least, stops, first, trail = _run(c, start, plan, table, .875)
            want['positions'][:, f, k], want['angles'][:, f, k], want['velocity'][:, f, k], want['angvelocity'][:, f, k] = (x[:, f] for x in st)
            want['progress'][:, f, k], want['stops'][:, f, k], want['first_stop'][:, f, k] = least[:, f], stops[:, f], first[:, f]
            want['trail'][:, f, k] = trail[:, f]
    _restore(c, start)
    _same(got, want)
    assert got.slides is None and (got.stops > 0).any() and (got.stops == 0).any()


def test_the_focal_mode_is_the_joint_call_on_the_expanded_tensor():
    from megastep_amd import cuda
    N, A, H = 5, 4, 3
    c, _ = _world(N, A, seed=14)
    _odd_poses(c, np.random.RandomState(15))
    _pair(c, 0, 2, 3)
    every, base, table = _plans(8, (N, A, 256, H)), _plans(9, (N, A, H)), _table()
    for K in (1, 16, 17, 256):
        plans_ = every[:, :, :K].contiguous()
        got = cuda.rollouts(c.scenery, c.agents, plans_, table, keep=.875, others=base, trail=True)
        joint = expanded(plans_, base)
        for f in range(A):                                               # (a joint call takes 256 scenarios: agent f's at a time)
            rows = cuda.scenarios(c.scenery, c.agents, joint[:, f*K:(f + 1)*K].contiguous(), table, keep=.875, trail=True)
            for k in FIELDS:
                util.assert_bits(getattr(got, k)[:, f].contiguous(), getattr(rows, k)[:, :, f].contiguous(), f'K = {K}, agent {f}: {k}')
    assert (got.stops > 0).any() and (got.stops == 0).any()


def test_idle_others_that_keep_nothing_are_others_at_rest():
    from megastep_amd import cuda
    N, A, K, H = 6, 3, 20, 4
    c, _ = _world(N, A, seed=16)
    _odd_poses(c, np.random.RandomState(17))
    _pair(c, 5, 0, 1)
    plans_, table = _plans(10, (N, A, K, H)), _table()
    base = torch.zeros((N, A, H), dtype=torch.int64, device='cuda')
    got = cuda.rollouts(c.scenery, c.agents, plans_, table, keep=0., others=base, trail=True)
    want = cuda.rollouts(c.scenery, c.agents, plans_, table, keep=0., others='rest', trail=True)
    _same(got, want)
    absent = cuda.rollouts(c.scenery, c.agents, plans_, table, keep=0., trail=True)
    assert not torch.equal(absent.stops[5], got.stops[5])


def test_call_plumbing():
    from megastep_amd import cuda, modules
    N, A, S, H = 6, 3, 20, 4
    c, _ = _world(N, A, seed=11)
    util.random_velocities(c, np.random.RandomState(12), speed=2.)
    _pair(c, 2, 0, 1)
    shared, table = _plans(5, (S, A, H)), _table()
    call = lambda **kw: cuda.scenarios(c.scenery, c.agents, shared, table, keep=.875, trail=True, **kw)
    before = _state(c)
    first = call()
    for x, y in zip(_state(c), before):
        util.assert_bits(x, y, 'the agents after a call')
    # (S, A, H) actions against the expanded tensor; the movement module's call
    _same(first, cuda.scenarios(c.scenery, c.agents, shared[None].expand(N, S, A, H).contiguous(), table, keep=.875, trail=True))
    assert first.trail.shape == (N, S, A, H, 2) and cuda.scenarios(c.scenery, c.agents, shared, table).trail is None
    mover = modules.MomentumMovement(c)
    _same(mover.scenarios(shared, trail=True), cuda.scenarios(c.scenery, c.agents, shared, mover._table, keep=mover.keep, trail=True))
    # mask (N,): without out the others read as not rolled; with out they keep what it held
    mask = torch.tensor([True, False, True, True, False, False], device='cuda')
    some = call(mask=mask)
    for k in FIELDS:
        util.assert_bits(getattr(some, k)[mask], getattr(first, k)[mask], k)
    assert torch.isnan(some.positions[~mask]).all() and torch.isnan(some.trail[~mask]).all() and (some.progress[~mask] == 1).all()
    assert (some.stops[~mask] == 0).all() and (some.first_stop[~mask] == H).all()
    held = {k: getattr(first, k).clone() for k in FIELDS}
    ptrs = [getattr(first, k).data_ptr() for k in FIELDS]
    util.random_velocities(c, np.random.RandomState(13), speed=2.)
    again = call(mask=mask, out=first)
    fresh = call()
    assert again is first and ptrs == [getattr(first, k).data_ptr() for k in FIELDS]
    for k in FIELDS:
        util.assert_bits(getattr(first, k)[mask], getattr(fresh, k)[mask], k)
        util.assert_bits(getattr(first, k)[~mask], held[k][~mask], k)
    with pytest.raises(RuntimeError, match='out'):
        cuda.scenarios(c.scenery, c.agents, shared[:5].contiguous(), table, keep=.875, trail=True, out=first)
    # the focal mode's mask (N, A) and out
    plans_, base = _plans(6, (8, H)), _plans(7, (N, A, H))
    focal = lambda **kw: cuda.rollouts(c.scenery, c.agents, plans_, table, keep=.875, others=base, trail=True, **kw)
    whole = focal()
    _same(whole, cuda.rollouts(c.scenery, c.agents, plans_[None, None].expand(N, A, 8, H).contiguous(), table, keep=.875, others=base, trail=True))
    fmask = torch.zeros((N, A), dtype=torch.bool, device='cuda')
    fmask[::2, 0] = True; fmask[1, 2] = True; fmask[2, 1] = True
    part = focal(mask=fmask)
    for k in FIELDS:
        util.assert_bits(getattr(part, k)[fmask], getattr(whole, k)[fmask], k)
    assert torch.isnan(part.positions[~fmask]).all() and (part.first_stop[~fmask] == H).all()
    assert focal(out=part) is part
    _same(part, whole)
    with pytest.raises(RuntimeError, match='slide'):
        focal(slide=True)
    # a side stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        aside = call()
    side.synchronize()
    _same(aside, fresh)
    # a captured call of each mode, replayed three times after the agents moved
    static, fstatic = call(), focal()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call(out=static)
        focal(out=fstatic)
    for replay in range(3):
        util.random_velocities(c, np.random.RandomState(14 + replay), speed=2.)
        c.agents.positions[:] = c.agents.positions + .05
        graph.replay()
        torch.cuda.synchronize()
        _same(static, call(), f'replay {replay}: ')
        _same(fstatic, focal(), f'replay {replay}, focal: ')
    assert not all(util.same_bits(getattr(static, k), getattr(fresh, k)).all() for k in ('positions', 'velocity'))


class _Anticipate:
    """An env whose step is the anticipating expert's: the decision handed in is ignored."""

    def __init__(self, env):
        self.env = env

    def __getattr__(self, name):
        return getattr(self.env, name)

    def step(self, decision):
        return self.env.step(self.env.expert('anticipate'))


def test_lookahead_among_repeating_others_takes_what_its_rule_says_of_its_own_rollouts():
    from megastep_amd import modules
    from megastep_amd.demo import PointGoal
    torch.manual_seed(3); np.random.seed(3)
    env = PointGoal(16, n_agents=3, geometries=plans(16), max_lifespan=10**6)
    env.reset()
    look = modules.LookAhead(env.core, env._goals, env._mover, others='repeat')
    assert look.base.shape == (16, 3, 8) and look.base.dtype == torch.int64 and (look.base == 0).all()
    assert modules.LookAhead(env.core, env._goals, env._mover).base is None
    held, chosen, last = look.base.data_ptr(), 0, torch.zeros((16, 3), dtype=torch.int64, device='cuda')
    for _ in range(6):
        assumed = look.base.clone()
        assert torch.equal(assumed, last[..., None].expand(16, 3, 8))    # (what the module returned at its previous call)
        decision = look()
        assert decision.actions.shape == (16, 3) and decision.actions.dtype == torch.int64
        action, none = modules.LookAhead.choose(look.values, look.rolled.stops, look.plans, look.stop_cost)
        assert torch.equal(look.values, env._goals.fields.at(look.rolled.positions.view(16, 3*49, 2), goal=look._agent).view(16, 3, 49))
        assert torch.equal(decision.actions[~none], action[~none])
        chosen += int((~none).sum())
        _same(look.rolled, env._mover.rollouts(look.plans, others=assumed))
        assert look.base.data_ptr() == held
        last = decision.actions.clone()
        env.step(decision)
    assert chosen > 3*48


def test_pointgoal_steps_under_the_anticipate_expert_eagerly_and_as_a_graph():
    from megastep_amd import arrdict, graphs
    from megastep_amd.demo import PointGoal
    logs = []
    for graphed in (False, True):
        torch.manual_seed(3); np.random.seed(3)
        env = PointGoal(16, n_agents=3, geometries=plans(16), max_lifespan=10**6)
        stepper = graphs.GraphedStep(_Anticipate(env), warmup=3) if graphed else _Anticipate(env)
        stepper.reset()
        env.expert('anticipate')                                         # (the expert and its buffers are made outside the graph)
        nothing = arrdict.arrdict(actions=torch.zeros((16, 3), dtype=torch.long, device='cuda'))
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
    assert env._anticipate.base is not None and env._lookahead is None
