"""Rollouts on the CPU: the serial host statement of the kernel's own per-step functions (ms_host_rollouts) against the rule over
the oracle's physics step (tests/rollout_rule.py), as bits in every output; cuda.plans against its definition; LookAhead.choose on
hand-made scores; the ABI; and the argument refusals, none of which may launch anything."""
import ctypes as C
import os
import re
import numpy as np
import pytest
import torch

from tests import util
from tests.rollout_rule import FIELDS, host_rollouts, rollout_rule, world_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RADIUS, FPS = .1, 10.
f = np.float32

# the seven actions of the movement modules at a brisk 3 m/s and 90 degrees a step ...
TABLE = f([[0, 0, 0], [0, 3, 0], [0, -3, 0], [3, 0, 0], [-3, 0, 0], [0, 0, 90], [0, 0, -90]])
# ... and with a row that takes 2 m a step: farther than any list of the wall grid reaches (1.3 m)
FAST = np.concatenate([TABLE, f([[0, 20, 0]])])


def _box(x0, y0, x1, y1):
    return [[x0, y0, x1, y0], [x1, y0, x1, y1], [x1, y1, x0, y1], [x0, y1, x0, y0]]


def _world(walls, positions, angles, velocity=None, angvelocity=None):
    positions = np.asarray(positions, f)
    N, A = positions.shape[:2]
    return dict(walls=[f(w).reshape(-1, 4) for w in walls], positions=positions, angles=np.asarray(angles, f).reshape(N, A),
                velocity=np.zeros((N, A, 2), f) if velocity is None else np.asarray(velocity, f).reshape(N, A, 2),
                angvelocity=np.zeros((N, A), f) if angvelocity is None else np.asarray(angvelocity, f).reshape(N, A))


def _plans(rng, shape, n_actions=7):
    return rng.randint(0, n_actions, shape).astype(np.int64)


def _hold(world, actions, table, keep, others=None, mask=None):
    """Both statements of one case, equal as bits in every output; returns the rule's."""
    want = rollout_rule(world, actions, table, keep, others, RADIUS, FPS, mask=mask)
    got = host_rollouts(world, actions, table, keep, others, RADIUS, FPS, mask=mask)
    for k in FIELDS:
        util.assert_bits(got[k], want[k], k)
    return want


def hand_worlds():
    """Two hand-made worlds of two envs each. The first: a corridor 0.5 m wide - narrower than two 0.3 m steps - with an agent
    in its middle, and a room with a pillar whose agent starts pressed against the west wall (a millimetre more than its radius
    off it). The second: an agent far outside its walls' box, and one crawling at 6e-7 m a step towards a wall."""
    corridor = _box(0, 0, 6, .5)
    room = _box(0, 0, 4, 4) + _box(1.5, 1.5, 2, 2) + [[3, 0, 4, 1]]
    first = _world([corridor, room], [[[1., .25]], [[.101, 2.]]], [[20.], [90.]])
    second = _world([room, room], [[[-30., 2.]], [[2.5, 1.45]]], [[0.], [180.]], velocity=[[[0., 0.]], [[-6e-6, 0.]]])
    return first, second


@pytest.mark.parametrize('keep', [0., .875])
def test_the_host_statement_is_the_rule_on_hand_made_worlds(oracle, keep):
    rng = np.random.RandomState(1)
    stopped, free = 0, 0
    for world in hand_worlds():
        want = _hold(world, _plans(rng, (2, 1, 14, 5)), TABLE, keep)
        stopped += (want['stops'] > 0).sum(); free += (want['stops'] == 0).sum()
    assert stopped > 3 and free > 3


def test_the_crawling_agent_is_stopped_by_walls_metres_away(oracle):
    """project()'s "+ 1e-6" at work (DESIGN 3.27 names it): the agent of the second world's second env, drifting at 6e-7 m a step
    with no action taken, is stopped by a wall it is nowhere near - and the host statement, behind its reach cull, agrees."""
    world = hand_worlds()[1]
    want = _hold(world, np.zeros((1, 1), np.int64), TABLE, 1.)
    assert want['stops'][1, 0, 0] == 1 and want['progress'][1, 0, 0] < 1


@pytest.mark.parametrize('keep', [0., .875])
def test_the_host_statement_is_the_rule_on_two_of_the_suites_plans(oracle, keep):
    c, _ = util.plan_world(2, 1, 8, 130, seed=3, device='cpu')
    world = world_of(c)
    rng = np.random.RandomState(2)
    world['velocity'] = rng.uniform(-3, 3, (2, 1, 2)).astype(f)
    want = _hold(world, _plans(rng, (2, 1, 10, 6)), TABLE, keep)
    assert (want['stops'] > 0).any() and (want['stops'] == 0).any()


def test_a_single_step_and_a_single_candidate(oracle):
    first, _ = hand_worlds()
    rng = np.random.RandomState(3)
    _hold(first, _plans(rng, (2, 1, 9, 1)), TABLE, .875)                  # H = 1
    _hold(first, _plans(rng, (2, 1, 1, 7)), TABLE, .875)                  # K = 1
    _hold(first, _plans(rng, (5, 4)), TABLE, 0.)                          # (K, H): the same plans for every agent


def test_actions_outside_the_table_are_clamped_and_a_row_too_fast_for_the_lists(oracle):
    first, _ = hand_worlds()
    actions = np.array([[-3, 7, 7, 1], [99, 0, 7, 7], [7, 7, 7, 7], [2**40, -2**40, 1, 1]], np.int64)
    want = _hold(first, actions, FAST, 0.)
    clamped = _hold(first, np.clip(actions, 0, 7), FAST, 0.)
    for k in FIELDS:
        util.assert_bits(want[k], clamped[k], k)
    assert (want['stops'] > 0).any()


@pytest.mark.parametrize('n_agents', [2, 4])
def test_the_other_agents_at_rest_are_obstacles(oracle, n_agents):
    """others='rest': agents 0 and 1 stand 0.21 m apart - within touching distance, 2.002 r - and the rest about the room; every
    agent's candidates meet the others where the call found them. Without others the same plans run through them."""
    room = _box(0, 0, 4, 4)
    spots = f([[1., 1.], [1.21, 1.], [3., 3.], [2., 3.2]])[:n_agents]
    world = _world([room], [spots], [[0., 90., 45., -90.][:n_agents]], velocity=np.zeros((1, n_agents, 2)))
    world['velocity'][0, 0] = [1., 0.]
    rng = np.random.RandomState(4)
    actions = _plans(rng, (1, n_agents, 8, 4))
    actions[0, 0, 0] = 3                                                  # agent 0 strafes along its heading's right ...
    actions[0, 1, 0] = [1, 2, 2, 0]                                       # ... and agent 1 steps straight at agent 0, and back
    rest = _hold(world, actions, TABLE, .875, others='rest')
    alone = _hold(world, actions, TABLE, .875)
    assert rest['stops'][0, 1, 0] > 0 and alone['stops'][0, 1, 0] == 0
    mask = np.zeros((1, n_agents), bool); mask[0, 1] = True
    masked = _hold(world, actions, TABLE, .875, others='rest', mask=mask)
    util.assert_bits(masked['positions'][0, 1], rest['positions'][0, 1])
    assert np.isnan(masked['positions'][0, 0]).all() and (masked['first_stop'][0, 0] == 4).all()


def test_plans_against_their_definition():
    from megastep_amd import cuda
    constant = cuda.plans(7, 8, switch=None)
    assert constant.dtype == torch.int64 and tuple(constant.shape) == (7, 8) and constant.is_contiguous()
    assert all((constant[i] == i).all() for i in range(7))
    p = cuda.plans(n_actions=7, horizon=8, switch=2)
    assert p.dtype == torch.int64 and tuple(p.shape) == (49, 8) and p.is_contiguous()
    for i in range(7):
        for j in range(7):
            assert p[i*7 + j].tolist() == [i]*2 + [j]*6
    assert cuda.plans(3, 4, switch=4).tolist() == [[i]*4 for i in range(3) for _ in range(3)]
    assert cuda.plans(3, 4, switch=0).tolist() == [[j]*4 for _ in range(3) for j in range(3)]
    for bad in (dict(n_actions=0, horizon=4), dict(n_actions=3, horizon=0), dict(n_actions=3, horizon=4, switch=5)):
        with pytest.raises(RuntimeError):
            cuda.plans(**bad)


def test_lookahead_choose_on_hand_made_scores():
    from megastep_amd.modules import LookAhead
    inf, nan = float('inf'), float('nan')
    plans = torch.tensor([[4, 0], [5, 0], [6, 0], [1, 0]])
    values = torch.tensor([[3., 2., 2., 5.],            # a tie: the lowest-numbered of the two
                           [inf, inf, inf, inf],        # nothing leads anywhere
                           [nan, 4., nan, 4.],          # NaNs score +inf; a tie behind them
                           [1., 1.5, 9., 1.],           # the stops decide: 1 + .5*2 against 1.5 + 0 against 1 + .5*1
                           [nan, nan, nan, nan],
                           [inf, 7., inf, nan]])
    stops = torch.tensor([[0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0], [2, 0, 0, 1], [0, 0, 0, 0], [0, 3, 0, 0]], dtype=torch.int32)
    action, none = LookAhead.choose(values, stops, plans, .5)
    assert action.dtype == torch.int64
    assert action.tolist() == [5, 4, 5, 5, 4, 5] and none.tolist() == [False, True, False, False, True, False]
    # per-agent plans, and leading axes
    each = plans[None].expand(6, 4, 2).flip(1).contiguous()
    action, none = LookAhead.choose(values.view(2, 3, 4), stops.view(2, 3, 4), each.view(2, 3, 4, 2), .5)
    assert action.tolist() == [[6, 1, 6], [6, 1, 6]] and none.tolist() == [[False, True, False], [False, True, False]]


def test_the_header_declares_the_call_and_the_abi_stands():
    from megastep_amd import _lib
    text = open(os.path.join(ROOT, 'include', 'megastep_hip.h')).read()
    assert re.search(r'\bint\s+ms_rollouts\s*\(', text) and re.search(r'^\}\s*MsRollouts\s*;', text, flags=re.M)
    assert int(re.search(r'#define\s+MS_ABI_VERSION\s+(\d+)', text).group(1)) == _lib.ABI_VERSION == 17
    assert _lib.lib().ms_abi_version() == 17
    test_text = open(os.path.join(ROOT, 'include', 'megastep_hip_test.h')).read()
    assert 'ms_host_rollouts' in test_text and 'ms_host_move_velocity' in test_text


def test_the_library_refuses_bad_rollouts_before_any_launch():
    """NULL pointers and zeroed structs only, and limits on a struct whose pointers are host memory: ms_rollouts returns before
    it gets as far as a launch (there is no device here to launch on), and the host statement refuses the same limits."""
    from megastep_amd import _lib
    h = _lib.lib()
    cfg = _lib.MsConfig(.1, 64, 130., 10.)
    sc, ag = _lib.MsScenery(), _lib.MsAgents()
    assert h.ms_rollouts(None, None, None, None, None) == -1
    assert h.ms_rollouts(C.byref(sc), C.byref(ag), C.byref(_lib.MsRollouts()), C.byref(cfg), None) == -1
    first, _ = hand_worlds()
    good = np.zeros((2, 1, 3, 4), np.int64)
    assert host_rollouts(first, good, TABLE, 0., None, RADIUS, FPS, raw=True) == 0
    for actions in (np.zeros((2, 1, 0, 4), np.int64), np.zeros((2, 1, 257, 4), np.int64), np.zeros((2, 1, 3, 65), np.int64),
                    np.zeros((2, 1, 3, 0), np.int64)):
        assert host_rollouts(first, actions, TABLE, 0., None, RADIUS, FPS, raw=True) == -1, actions.shape
    assert host_rollouts(first, good, TABLE[:0], 0., None, RADIUS, FPS, raw=True) == -1                  # n_actions = 0
    assert host_rollouts(first, good, TABLE, float('nan'), None, RADIUS, FPS, raw=True) == -1


def test_the_call_refuses_bad_arguments_before_any_launch():
    """The Python surface: every refusal below is raised on CPU tensors, ahead of the device check - shapes, dtypes, limits and
    contiguity are settled before there is anything to launch on - and a well-formed call on CPU tensors then asks for a GPU."""
    from megastep_amd import cuda
    c, _ = util.plan_world(1, 2, 8, 130, toy='box', device='cpu')
    table = torch.as_tensor(TABLE)
    acts = lambda *shape: torch.zeros(shape, dtype=torch.int64)
    call = lambda actions, table=table, **kw: cuda.rollouts(c.scenery, c.agents, actions, table, **kw)
    for actions, match in ((acts(0, 8), 'K must be'), (acts(257, 8), 'K must be'), (acts(4, 65), 'H must be'), (acts(4, 0), 'H must be'),
                           (acts(1, 2, 0, 8), 'K must be'), (acts(4, 8).int(), 'dtype'), (acts(4, 8).float(), 'dtype'),
                           (acts(3, 2, 4, 8), 'actions must be'), (acts(1, 4, 8), 'actions must be'), (acts(8, 4).t(), 'contiguous'),
                           ([[0, 1]], 'actions must be')):
        with pytest.raises(RuntimeError, match=match):
            call(actions)
    with pytest.raises(RuntimeError, match='dtype'):
        call(acts(4, 8), table.double())
    with pytest.raises(RuntimeError, match='n_actions, 3'):
        call(acts(4, 8), table[:, :2].contiguous())
    with pytest.raises(RuntimeError, match='n_actions, 3'):
        call(acts(4, 8), table[:0])
    with pytest.raises(RuntimeError, match='others'):
        call(acts(4, 8), others='all')
    with pytest.raises(RuntimeError, match='mask'):
        call(acts(4, 8), mask=torch.ones((1, 3), dtype=torch.bool))
    with pytest.raises(RuntimeError, match='dtype'):
        call(acts(4, 8), mask=torch.ones((1, 2)))
    with pytest.raises(RuntimeError, match='GPU'):
        call(acts(4, 8))
