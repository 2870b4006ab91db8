"""Scenarios on the CPU: the serial host statement of the kernel's own per-step functions (ms_host_scenarios) against the rule over
the oracle's physics step (tests/scenario_rule.py), as bits in every output; the hand-made meetings the feature exists for; the
focal mode against the joint one; the degenerate cases against the rollouts' rule; the ABI; the refusals, none of which may
launch anything; and LookAhead(others='repeat')'s buffer rule."""
import ctypes as C
import os
import re
import numpy as np
import pytest
import torch

from tests import util
from tests.rollout_rule import FIELDS, rollout_rule, world_of
from tests.scenario_rule import expand_focal, focal_rows, host_scenarios, scenario_rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RADIUS, FPS = .1, 10.
f = np.float32

# the seven actions of the movement modules at a brisk 3 m/s - 0.3 m a step - and 90 degrees a step: at angle 0 action 1 walks
# towards +y, at -90 towards +x, at 90 towards -x ...
TABLE = f([[0, 0, 0], [0, 3, 0], [0, -3, 0], [3, 0, 0], [-3, 0, 0], [0, 0, 90], [0, 0, -90]])
# ... and with a row that takes 2 m a step: farther than any list of the wall grid reaches (1.3 m)
FAST = np.concatenate([TABLE, f([[0, 20, 0]])])
EAST, WEST, NORTH = -90., 90., 0.


def _box(x0, y0, x1, y1):
    return [[x0, y0, x1, y0], [x1, y0, x1, y1], [x1, y1, x0, y1], [x0, y1, x0, y0]]


ROOM = _box(0, 0, 4, 4)
PILLAR = ROOM + _box(1.5, 1.5, 2, 2) + [[3, 0, 4, 1]]


def _world(walls, positions, angles, velocity=None, angvelocity=None):
    positions = np.asarray(positions, f)
    N, A = positions.shape[:2]
    return dict(walls=[f(w).reshape(-1, 4) for w in walls], positions=positions, angles=np.asarray(angles, f).reshape(N, A),
                velocity=np.zeros((N, A, 2), f) if velocity is None else np.asarray(velocity, f).reshape(N, A, 2),
                angvelocity=np.zeros((N, A), f) if angvelocity is None else np.asarray(angvelocity, f).reshape(N, A))


def _plans(rng, shape, n_actions=7):
    return rng.randint(0, n_actions, shape).astype(np.int64)


def _same(got, want):
    for k in FIELDS:
        util.assert_bits(got[k], want[k], k)


def _hold(world, actions, table, keep, mask=None):
    """Both statements of one joint case, equal as bits in all eight outputs; returns the rule's."""
    want = scenario_rule(world, actions, table, keep, RADIUS, FPS, mask=mask)
    _same(host_scenarios(world, actions, table, keep, RADIUS, FPS, mask=mask), want)
    return want


def _walk(*per_agent, horizon):
    """(1, 1, A, H): one env, one scenario, agent a taking per_agent[a] at every step."""
    return np.array(per_agent, np.int64)[None, None, :, None].repeat(horizon, 3)


# ----------------------------------------------------------------------------------------------------------------------
# the meetings
# ----------------------------------------------------------------------------------------------------------------------
def test_two_agents_head_on_in_a_corridor_stop_each_other(oracle):
    """A corridor 0.5 m wide; two agents 0.5 m apart walk at each other, 0.3 m a step each: both are stopped dead at step 0."""
    world = _world([_box(0, 0, 6, .5)], [[[2., .25], [2.5, .25]]], [[EAST, WEST]])
    want = _hold(world, _walk(1, 1, horizon=3), TABLE, 0.)
    assert (want['first_stop'][0, 0] == 0).all() and (want['progress'][0, 0] < 1).all()
    assert (want['velocity'][0, 0] == 0).all()


def test_a_follower_is_not_blocked_by_a_body_that_moves_out_of_its_way(oracle):
    """The case the feature exists for, as a difference: one agent 0.25 m behind another, both walking east at 0.3 m a step.
    In the scenario NEITHER is stopped; the rollouts' rule with the others at rest stops the follower."""
    world = _world([ROOM], [[[1., 3.], [1.25, 3.]]], [[EAST, EAST]])
    want = _hold(world, _walk(1, 1, horizon=3), TABLE, 0.)
    assert (want['stops'][0, 0] == 0).all() and (want['progress'][0, 0] == 1).all()
    np.testing.assert_allclose(want['positions'][0, 0, :, 0], [1.9, 2.15], atol=1e-5)
    rest = rollout_rule(world, np.ones((1, 3), np.int64), TABLE, 0., 'rest', RADIUS, FPS)
    assert rest['stops'][0, 0, 0] > 0 and rest['first_stop'][0, 0, 0] == 0


def test_two_paths_crossing_at_right_angles(oracle):
    """One walks east, one north, to meet at (1.6, 2) in the second step: both are stopped there, not in the first."""
    world = _world([ROOM], [[[1., 2.], [1.6, 1.4]]], [[EAST, NORTH]])
    want = _hold(world, _walk(1, 1, horizon=3), TABLE, 0.)
    assert (want['first_stop'][0, 0] == 1).all()


@pytest.mark.parametrize('keep', [0., .875])
def test_three_bodies_touching_and_one_pressed_to_a_wall_while_pushed(oracle, keep):
    """Env 0: three discs within touching distance (2.002 r) of each other. Env 1: one pressed flat to the west wall, a
    millimetre more than its radius off it, another walking into it from the east. Random plans on top of the meetings."""
    world = _world([PILLAR, ROOM], [[[2.5, 2.5], [2.7, 2.5], [2.6, 2.67]], [[.101, 2.], [.31, 2.], [3., 3.]]],
                   [[EAST, WEST, 180.], [WEST, WEST, 45.]])
    rng = np.random.RandomState(5)
    actions = _plans(rng, (2, 6, 3, 4))
    actions[:, 0] = 1                                                     # everybody straight ahead
    actions[1, 1, 0], actions[1, 1, 1] = 0, 1                             # the pressed one idle, still pushed
    want = _hold(world, actions, TABLE, keep)
    assert (want['stops'][0, 0] > 0).all() and (want['stops'][1, 0, :2] > 0).all() and want['stops'][1, 1, 1] > 0
    assert (want['stops'] == 0).any()


def test_a_nan_pose_among_sound_agents(oracle):
    nan = float('nan')
    world = _world([PILLAR], [[[nan, nan], [1., 1.], [1.21, 1.], [3., 3.]]], [[0., EAST, WEST, nan]])
    rng = np.random.RandomState(6)
    want = _hold(world, _plans(rng, (1, 5, 4, 3)), TABLE, .875)
    assert np.isnan(want['positions'][0, :, 0]).all() and not np.isnan(want['positions'][0, :, 1:3]).any()


@pytest.mark.parametrize('keep', [0., .875])
def test_far_outside_too_fast_for_the_lists_and_crawling(oracle, keep):
    """An agent 30 m outside its walls, one that may take the row of 2 m a step, and one drifting at 6e-7 m a step."""
    world = _world([PILLAR], [[[-30., 2.], [1., 1.], [2.5, 1.45]]], [[0., 0., 180.]], velocity=[[[0., 0.], [0., 0.], [-6e-6, 0.]]])
    rng = np.random.RandomState(7)
    actions = _plans(rng, (1, 7, 3, 4), n_actions=8)
    actions[0, 0, 1] = 7
    want = _hold(world, actions, FAST, keep)
    assert (want['stops'] > 0).any() and (want['stops'] == 0).any()


def test_the_crawling_agent_is_stopped_and_its_neighbour_is_not(oracle):
    """project()'s "+ 1e-6"  among several agents: the crawler, no action taken and keep 1, is stopped by walls it
    is nowhere near; the agent beside it stands still and is not."""
    world = _world([PILLAR], [[[2.5, 1.45], [3., 3.]]], [[180., 0.]], velocity=[[[-6e-6, 0.], [0., 0.]]])
    want = _hold(world, _walk(0, 0, horizon=1), TABLE, 1.)
    assert want['stops'][0, 0, 0] == 1 and want['stops'][0, 0, 1] == 0


@pytest.mark.parametrize('keep', [0., .875])
def test_the_host_statement_is_the_rule_on_two_of_the_suites_plans(oracle, keep):
    c, _ = util.plan_world(2, 3, 8, 130, seed=3, device='cpu')
    world = world_of(c)
    rng = np.random.RandomState(2)
    world['velocity'] = rng.uniform(-3, 3, (2, 3, 2)).astype(f)
    world['positions'][:, 1] = world['positions'][:, 0] + f([.22, .05])  # (a pair a step apart in each env)
    want = _hold(world, _plans(rng, (2, 6, 3, 5)), TABLE, keep)
    assert (want['stops'] > 0).any() and (want['stops'] == 0).any()


# ----------------------------------------------------------------------------------------------------------------------
# shapes
# ----------------------------------------------------------------------------------------------------------------------
def _crowd(n_agents, rng):
    """n_agents in an 8 m room, on a 0.21 m lattice in its middle: neighbours a step and less apart."""
    side = int(np.ceil(np.sqrt(n_agents)))
    spots = f([[3. + .21*(i % side), 3. + .21*(i//side)] for i in range(n_agents)])
    return _world([_box(0, 0, 8, 8)], [spots], [rng.uniform(-180, 180, n_agents)])


@pytest.mark.parametrize('n_agents, S, H', [(1, 4, 3), (2, 5, 3), (3, 4, 3), (5, 3, 3), (64, 2, 2)])
def test_agents_an_env_from_one_to_sixty_four(oracle, n_agents, S, H):
    rng = np.random.RandomState(n_agents)
    world = _crowd(n_agents, rng)
    want = _hold(world, _plans(rng, (1, S, n_agents, H)), TABLE, .875)
    if n_agents > 1:
        assert (want['stops'] > 0).any()


def test_a_single_step_a_single_scenario_shared_actions_and_a_mask(oracle):
    world = _world([PILLAR, ROOM], [[[1., 1.], [1.21, 1.]], [[.101, 2.], [3., 3.]]], [[EAST, WEST], [WEST, 0.]])
    rng = np.random.RandomState(3)
    _hold(world, _plans(rng, (2, 6, 2, 1)), TABLE, .875)                  # H = 1
    _hold(world, _plans(rng, (2, 1, 2, 6)), TABLE, .875)                  # S = 1
    shared = _plans(rng, (5, 2, 4))
    want = _hold(world, shared, TABLE, 0.)                                # (S, A, H): the same scenarios for every env
    _same(want, scenario_rule(world, np.broadcast_to(shared, (2, 5, 2, 4)), TABLE, 0., RADIUS, FPS))
    masked = _hold(world, shared, TABLE, 0., mask=np.array([False, True]))
    util.assert_bits(masked['positions'][1], want['positions'][1])
    assert np.isnan(masked['positions'][0]).all() and (masked['first_stop'][0] == 4).all() and (masked['progress'][0] == 1).all()


def test_actions_far_outside_the_table_are_clamped(oracle):
    world = _world([PILLAR], [[[1., 1.], [1.21, 1.]]], [[EAST, WEST]])
    actions = np.array([[[-3, 7, 7, 1], [99, 0, 7, 7]], [[7, 7, 7, 7], [2**40, -2**40, 1, 1]]], np.int64)[None]
    want = _hold(world, actions, FAST, 0.)
    _same(want, _hold(world, np.clip(actions, 0, 7), FAST, 0.))
    assert (want['stops'] > 0).any()


# ----------------------------------------------------------------------------------------------------------------------
# the rule against the rules there were
# ----------------------------------------------------------------------------------------------------------------------
def test_one_agent_an_env_is_the_rollouts_rule(oracle):
    world = _world([_box(0, 0, 6, .5), PILLAR], [[[1., .25]], [[.101, 2.]]], [[20.], [90.]])
    rng = np.random.RandomState(8)
    actions = _plans(rng, (2, 9, 1, 5))
    got = host_scenarios(world, actions, TABLE, .875, RADIUS, FPS)
    want = rollout_rule(world, actions.transpose(0, 2, 1, 3), TABLE, .875, None, RADIUS, FPS)
    for k in FIELDS:
        util.assert_bits(np.swapaxes(got[k], 1, 2), want[k], k)
    assert (want['stops'] > 0).any()


@pytest.mark.parametrize('shared', [False, True])
def test_focal_mode_is_joint_mode_on_the_expanded_tensor(oracle, shared):
    world = _world([PILLAR, ROOM], [[[1., 1.], [1.21, 1.], [3., 3.]], [[.101, 2.], [.31, 2.], [2., 3.2]]],
                   [[EAST, WEST, 0.], [WEST, WEST, 45.]], velocity=np.random.RandomState(1).uniform(-2, 2, (2, 3, 2)))
    rng = np.random.RandomState(9)
    plans = _plans(rng, (5, 4) if shared else (2, 3, 5, 4))
    base = _plans(rng, (2, 3, 4))
    joint = expand_focal(plans, base, 2, 3)
    assert joint.shape == (2, 15, 3, 4)
    want = focal_rows(scenario_rule(world, joint, TABLE, .875, RADIUS, FPS), 3)
    _same(focal_rows(host_scenarios(world, joint, TABLE, .875, RADIUS, FPS), 3), want)
    _same(host_scenarios(world, plans, TABLE, .875, RADIUS, FPS, base=base), want)
    mask = np.array([[True, False, True], [False, True, False]])
    masked = host_scenarios(world, plans, TABLE, .875, RADIUS, FPS, base=base, mask=mask)
    util.assert_bits(masked['positions'][mask], want['positions'][mask])
    assert np.isnan(masked['positions'][~mask]).all() and (masked['first_stop'][~mask] == 4).all()
    assert (want['stops'] > 0).any() and (want['stops'] == 0).any()


def test_idle_others_that_keep_nothing_are_others_at_rest(oracle):
    """keep = 0 and an all-no-op base: the others stand where they are with no velocity - rollout_rule(others='rest')."""
    world = _world([ROOM], [[[1., 1.], [1.21, 1.], [3., 3.], [2., 3.2]]], [[0., 90., 45., -90.]],
                   velocity=np.random.RandomState(2).uniform(-2, 2, (1, 4, 2)))
    rng = np.random.RandomState(4)
    plans = _plans(rng, (1, 4, 8, 4))
    plans[0, 1, 0] = [1, 2, 2, 0]
    got = host_scenarios(world, plans, TABLE, 0., RADIUS, FPS, base=np.zeros((1, 4, 4), np.int64))
    want = rollout_rule(world, plans, TABLE, 0., 'rest', RADIUS, FPS)
    _same(got, want)
    assert want['stops'][0, 1, 0] > 0


# ----------------------------------------------------------------------------------------------------------------------
# the ABI, the refusals, the modules
# ----------------------------------------------------------------------------------------------------------------------
def test_the_header_declares_the_call_and_the_abi_stands():
    from megastep_amd import _lib
    text = open(os.path.join(ROOT, 'include', 'megastep_hip.h')).read()
    assert re.search(r'\bint\s+ms_scenarios\s*\(', text) and re.search(r'^\}\s*MsScenarios\s*;', text, flags=re.M)
    assert 'kernels.cu:179-230' in text[text.index('Scenarios: whole envs'):text.index('} MsScenarios;')]
    assert int(re.search(r'#define\s+MS_ABI_VERSION\s+(\d+)', text).group(1)) == _lib.ABI_VERSION == 17
    assert _lib.lib().ms_abi_version() == 17
    assert 'ms_host_scenarios' in open(os.path.join(ROOT, 'include', 'megastep_hip_test.h')).read()
    # the binding lays the struct out as the header does: field for field
    body = text[text.index('typedef struct MsScenarios {'):text.index('} MsScenarios;')]
    names = re.findall(r'(\w+);', re.sub(r'/\*.*?\*/', '', body, flags=re.S))
    assert names == [name for name, _ in _lib.MsScenarios._fields_]


def test_the_library_refuses_bad_scenarios_before_any_launch():
    """The host statement refuses every limit; ms_scenarios refuses NULLs and zeroed structs, and - on structs whose pointers
    are HOST memory, every one with exactly one defect - each limit, each alignment and a wall grid given in part, with the
    code of an argument check: it returned before it got as far as a launch."""
    from megastep_amd import _lib
    h = _lib.lib()
    EINVAL, EUNSUPPORTED = -1, -3
    world = _world([PILLAR], [[[1., 1.], [1.21, 1.]]], [[EAST, WEST]])
    run = lambda actions, table=TABLE, keep=0., **kw: host_scenarios(world, actions, table, keep, RADIUS, FPS, raw=True, **kw)
    good = np.zeros((1, 3, 2, 4), np.int64)
    assert run(good) == 0
    for shape in ((1, 0, 2, 4), (1, 257, 2, 4), (1, 3, 2, 65), (1, 3, 2, 0)):
        assert run(np.zeros(shape, np.int64)) == EINVAL, shape
    assert run(good, table=TABLE[:0]) == EINVAL
    assert run(good, keep=float('nan')) == EINVAL
    plans, base = np.zeros((3, 4), np.int64), np.zeros((1, 2, 4), np.int64)
    assert run(plans, base=base) == 0
    assert run(np.zeros((257, 4), np.int64), base=base) == EINVAL and run(np.zeros((0, 4), np.int64), base=base) == EINVAL

    def without(name, value=None):
        return lambda q: setattr(q, name, value)
    for name in ('actions', 'table', 'positions', 'angles', 'velocity', 'angvelocity', 'progress', 'stops', 'first_stop'):
        assert run(good, edit=without(name)) == EINVAL, name
    assert run(plans, base=base, edit=without('base')) == EINVAL
    assert run(good, edit=without('focal', 2)) == EINVAL and run(good, edit=without('shared', -1)) == EINVAL
    crowd = _world([ROOM], [np.zeros((65, 2))], [np.zeros(65)])
    assert host_scenarios(crowd, np.zeros((1, 1, 65, 1), np.int64), TABLE, 0., RADIUS, FPS, raw=True) == EUNSUPPORTED

    # the device call, never as far as a launch
    cfg = _lib.MsConfig(.1, 64, 130., 10.)
    assert h.ms_scenarios(None, None, None, None, None) == EINVAL
    assert h.ms_scenarios(C.byref(_lib.MsScenery()), C.byref(_lib.MsAgents()), C.byref(_lib.MsScenarios()), C.byref(cfg), None) == EINVAL
    mem = np.zeros(4096, np.uint8)
    at = (mem.ctypes.data + 63)//64*64                                    # host memory, 64-byte aligned

    def call(defect, n_agents=2):
        sc = _lib.MsScenery()
        sc.n_envs, sc.n_agents, sc.n_model = 1, n_agents, 4
        sc.lines_vals = sc.lines_widths = sc.lines_starts = sc.model = at
        ag = _lib.MsAgents(at, at, at, at, None, None)
        q = _lib.MsScenarios(3, 4, 0, at, 0, None, at, 7, 0., None, at, at, at, at, at, at, at, None)
        defect(sc, ag, q)
        return h.ms_scenarios(C.byref(sc), C.byref(ag), C.byref(q), C.byref(cfg), None)
    q_is = lambda name, value: lambda sc, ag, q: setattr(q, name, value)
    for name, value in (('n_scenarios', 0), ('n_scenarios', 257), ('horizon', 0), ('horizon', 65), ('n_actions', 0), ('keep', float('nan')),
                        ('focal', 1), ('actions', None), ('table', None), ('first_stop', None), ('actions', at + 4), ('positions', at + 4),
                        ('velocity', at + 4), ('trail', at + 4), ('angles', at + 2), ('stops', at + 1)):
        assert call(q_is(name, value)) == EINVAL, (name, value)
    assert call(lambda sc, ag, q: setattr(ag, 'positions', at + 4)) == EINVAL
    assert call(lambda sc, ag, q: setattr(ag, 'velocity', None)) == EINVAL
    assert call(lambda sc, ag, q: setattr(sc, 'wg_cells', at)) == EINVAL                                # a wall grid given in part
    assert call(lambda sc, ag, q: None, n_agents=65) == EUNSUPPORTED


def test_the_calls_refuse_bad_arguments_before_any_launch():
    """The Python surface on CPU tensors, ahead of the device check; a well-formed call then asks for a GPU."""
    from megastep_amd import cuda, modules
    c, _ = util.plan_world(1, 2, 8, 130, toy='box', device='cpu')
    table = torch.as_tensor(TABLE)
    acts = lambda *shape: torch.zeros(shape, dtype=torch.int64)
    call = lambda actions, table=table, **kw: cuda.scenarios(c.scenery, c.agents, actions, table, **kw)
    for actions, match in ((acts(0, 2, 8), 'S must be'), (acts(257, 2, 8), 'S must be'), (acts(4, 2, 65), 'H must be'), (acts(4, 2, 0), 'H must be'),
                           (acts(4, 3, 8), 'actions must be'), (acts(2, 4, 2, 8), 'actions must be'), (acts(4, 8), 'actions must be'),
                           (acts(4, 2, 8).int(), 'dtype'), (acts(8, 2, 4).transpose(0, 2), 'contiguous'), ([[[0, 1]]], 'actions must be')):
        with pytest.raises(RuntimeError, match=match):
            call(actions)
    with pytest.raises(RuntimeError, match='n_actions, 3'):
        call(acts(4, 2, 8), table[:0])
    with pytest.raises(RuntimeError, match='keep'):
        call(acts(4, 2, 8), keep=float('nan'))
    with pytest.raises(RuntimeError, match='mask'):
        call(acts(4, 2, 8), mask=torch.ones((1, 2), dtype=torch.bool))
    with pytest.raises(RuntimeError, match='GPU'):
        call(acts(4, 2, 8))
    # the focal mode, through cuda.rollouts
    roll = lambda others, actions=acts(4, 8), **kw: cuda.rollouts(c.scenery, c.agents, actions, table, others=others, **kw)
    for others, match in ((acts(1, 2, 7), 'others must be'), (acts(2, 8), 'others'), (acts(1, 2, 8).int(), 'dtype')):
        with pytest.raises(RuntimeError, match=match):
            roll(others)
    with pytest.raises(RuntimeError, match='slide'):
        roll(acts(1, 2, 8), slide=True)
    with pytest.raises(RuntimeError, match='mask'):
        roll(acts(1, 2, 8), mask=torch.ones((1,), dtype=torch.bool))
    with pytest.raises(RuntimeError, match='GPU'):
        roll(acts(1, 2, 8))
    with pytest.raises(RuntimeError, match='GPU'):
        modules.MomentumMovement(c).scenarios(acts(4, 2, 8))
    with pytest.raises(RuntimeError, match='slid'):
        modules.SimpleMovement(c, slide=True).scenarios(acts(4, 2, 8))
    with pytest.raises(RuntimeError, match="'rest' or 'repeat'"):
        modules.LookAhead(c, None, modules.MomentumMovement(c), others='all')


def test_the_repeat_rule_of_lookahead_on_plain_tensors():
    """others='repeat': the buffer holds, at every step of the horizon, the action the module last returned - written in place."""
    from megastep_amd.modules import LookAhead
    base = torch.zeros((2, 3, 4), dtype=torch.int64)
    held = base.data_ptr()
    actions = torch.tensor([[4, 0, 6], [1, 2, 3]])
    back = LookAhead.repeat(base, actions)
    assert back is base and base.data_ptr() == held
    assert base.tolist() == [[[4]*4, [0]*4, [6]*4], [[1]*4, [2]*4, [3]*4]]
    LookAhead.repeat(base, torch.tensor([[5, 5, 5], [0, 0, 0]]))
    assert base[0].eq(5).all() and base[1].eq(0).all() and base.data_ptr() == held
