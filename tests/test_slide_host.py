"""Sliding contacts on the CPU: the serial host statement of the kernel's own per-agent functions (ms_host_slide)
against the numpy restatement of the rule around the oracle's collision tests (tests/slide_rule.py), as bits in every output; the
invariants that tie the sliding step to the plain one; that it does slide; that it crosses no wall; and the argument refusals."""
import ctypes as C
import numpy as np
import pytest

from tests import util
from tests.slide_rule import FIELDS, STATE, advance, host_slide, plain_rule, plain_scene, slide_rule, world, _cs, _moved

RADIUS, FPS = .106, 10.
f = np.float32
# the movement modules' seven actions at a brisk 3 m/s and 90 degrees a step ...
TABLE = f([[0, 0, 0], [0, 3, 0], [0, -3, 0], [3, 0, 0], [-3, 0, 0], [0, 0, 90], [0, 0, -90]])
# ... and a momentum agent's: half a metre a second and 40 degrees a second more each step
GENTLE = f([[0, 0, 0], [0, .5, 0], [0, -.5, 0], [.5, 0, 0], [-.5, 0, 0], [0, 0, 40], [0, 0, -40]])
LONG_WALL = [[0, 0, 20, 0]]
CONVEX_L = [[0, 0, 10, 0], [10, 0, 10, -10]]
CONCAVE = [[0, 0, 10, 0], [10, 0, 10, 10]]


def _box(x0, y0, x1, y1):
    return [[x0, y0, x1, y0], [x1, y0, x1, y1], [x1, y1, x0, y1], [x0, y1, x0, y0]]


def push(degrees, speed=.5):
    """A one-row table: `speed` more each step at a fixed world angle, for agents that keep heading 0 (sin 0 and cos 0 are exact)."""
    a = np.deg2rad(degrees)
    return f([[speed*np.cos(a), speed*np.sin(a), 0.]])


def hold(w, bounce=.05, movement=None, scene=None):
    """One step of both statements, equal as bits in every output, and the invariants: `progress` is the plain step's, and an env
    in which nobody was blocked is the plain step's in every output. Returns the rule's outputs."""
    want = slide_rule(w, RADIUS, FPS, bounce, movement)
    got = host_slide(w, RADIUS, FPS, bounce, movement)
    for k in FIELDS:
        util.assert_bits(got[k], want[k], k)
    plain = plain_rule(w, RADIUS, FPS, movement, scene=scene)
    util.assert_bits(want['progress'], plain['progress'], 'progress')
    free = (want['progress'] >= 1).all(1)
    for k in STATE:
        util.assert_bits(want[k][free], plain[k][free], k)
    assert not want['stopped'][free].any() and not want['slid'][free].any()
    return want


def walk(w, steps, bounce=.05, table=None, keep=.875, actions=None):
    """`steps` steps of hold(): the dead stops, the steps that slid, and the world it ends in."""
    stops = slid = 0
    scene = plain_scene(w)
    for h in range(steps):
        movement = None if table is None else (np.zeros(w['angles'].shape, np.int64) if actions is None else actions[h], table, keep)
        out = hold(w, bounce, movement, scene)
        stops += int(out['stopped'].sum()); slid += int((out['slid'] > 0).sum())
        w = advance(w, out)
    return stops, slid, w


def plain_walk(w, steps, table, keep=.875):
    stops = 0
    scene = plain_scene(w)
    for h in range(steps):
        out = plain_rule(w, RADIUS, FPS, (np.zeros(w['angles'].shape, np.int64), table, keep), scene=scene)
        stops += int((out['progress'] < 1).sum())
        w = advance(w, out)
    return stops, w


@pytest.mark.parametrize('degrees', [-45, -10, -80])
@pytest.mark.parametrize('walls', [LONG_WALL, CONVEX_L], ids=['long-wall', 'convex-L'])
def test_the_host_statement_is_the_rule_along_a_wall(oracle, walls, degrees):
    start = [[[1.3, .5]]] if walls is LONG_WALL else [[[6., .5]]]
    stops, slid, _ = walk(world([walls], start), 60, table=push(degrees))
    assert slid > 5


@pytest.mark.parametrize('bounce', [0., .05, 1.])
def test_the_host_statement_is_the_rule_at_every_bounce(oracle, bounce):
    stops, slid, _ = walk(world([LONG_WALL], [[[1.3, .5]]]), 40, bounce=bounce, table=push(-45))
    assert stops + slid > 10


def test_it_slides_where_the_plain_step_sticks(oracle):
    """The condition the rule was taken up on: a momentum agent pushed at -80 degrees against the long wall for 120 steps. The plain
    step stops it dead nearly every step; the sliding step hardly ever, and carries it metres along the wall."""
    w = world([LONG_WALL], [[[1.3, .5]]])
    plain_stops, plain_end = plain_walk(w, 120, push(-80))
    stops, slid, end = walk(w, 120, table=push(-80))
    print(f'plain: {plain_stops} dead stops, x = {plain_end["positions"][0, 0, 0]:.2f}; slide: {stops} dead stops, {slid} slides, '
          f'x = {end["positions"][0, 0, 0]:.2f}')
    assert plain_stops >= 100
    assert stops <= 5 and end['positions'][0, 0, 0] > 5


def test_a_concave_corner_pushed_into_is_a_dead_stop_in_phase_b(oracle):
    w = world([CONCAVE], [[[9.5, .5]]])
    stopped_in_b = 0
    for h in range(30):
        out = hold(w, movement=(np.zeros((1, 1), np.int64), push(-20), .875))
        stopped_in_b += int(out['stopped'][0, 0] and out['slid'][0, 0] > 0)
        w = advance(w, out)
    assert stopped_in_b > 0


def test_a_corridor_narrower_than_two_steps(oracle):
    w = world([_box(0, 0, 6, .5)], [[[1., .25]]], angles=[[20.]])
    rng = np.random.RandomState(1)
    stops, slid, _ = walk(w, 30, table=TABLE, keep=0., actions=rng.randint(0, 7, (30, 1, 1)))
    assert slid > 0


def test_an_agent_pressed_flat_on_a_wall(oracle):
    """x1 = 0: the agent stands within 1.001 R of the wall and moves into it - phase A grants nothing, phase B the whole step."""
    w = world([LONG_WALL], [[[5., .106]]], velocity=[[[1., -1.]]])
    out = hold(w)
    assert out['progress'][0, 0] == 0 and out['slid'][0, 0] > 0


def test_two_walls_of_equal_value_and_different_normals(oracle):
    """A symmetric notch met head-on: both walls give the same x1, bit for bit, and mirror-image normals - the least key decides,
    whichever order the rows come in - and the same wall listed twice changes nothing."""
    notch = [[0, 0, -2, 2], [0, 0, 2, 2]]
    outs = []
    for rows in (notch, notch[::-1], notch + notch[:1], notch[1:] + notch):
        w = world([rows], [[[0., 1.]]], velocity=[[[0., -9.]]])
        u = (f(0), f(f(-9.)/f(FPS)))
        assert _cs(w['positions'][0, 0], u, f(notch[0]), f(RADIUS)) == _cs(w['positions'][0, 0], u, f(notch[1]), f(RADIUS)) < 1
        outs.append(hold(w))
    for o in outs[1:]:
        for k in FIELDS:
            util.assert_bits(o[k], outs[0][k], k)
    assert outs[0]['progress'][0, 0] < 1


def test_rows_that_are_no_walls_and_a_pose_that_is_none(oracle):
    """A zero-length row, a NaN row and a NaN pose: passed over, never a winner; the agents beside them step as ever."""
    nan = float('nan')
    rows = LONG_WALL + [[3, .05, 3, .05], [nan, 1, 2, nan], [4, nan, 5, 0]]
    w = world([rows, rows], [[[2.9, .3], [7., .4]], [[nan, 1.], [12., nan]]], velocity=[[[.5, -2.], [1., -3.]], [[1., 1.], [0., -1.]]])
    out = hold(w)
    assert out['slid'][0].all() and not out['slid'][1].any()
    # ... and standing ON the zero-length row: its offset has no length
    w = world([[[3, .05, 3, .05]]], [[[3., .05]]], velocity=[[[1., 0.]]])
    hold(w)


@pytest.mark.parametrize('n_agents', [2, 4])
def test_agents_within_touching_distance(oracle, n_agents):
    """Agents 0 and 1 stand 0.25 m apart, 2.36 R: 0 runs into 1, which the wall below both has stopped by then - one blocked by the
    other, both sliding; the others about the room."""
    spots = f([[1., .12], [1.25, .12], [3., 3.], [2., 3.2]])[:n_agents]
    vel = f([[2., 0.], [.5, -2.], [0., 0.], [-1., -1.]])[:n_agents]
    w = world([_box(0, 0, 4, 4)], [spots], velocity=[vel])
    out = hold(w)
    assert out['progress'][0, 0] < 1 and out['progress'][0, 1] < 1 and out['slid'][0, :2].all()
    for h in range(10):
        w = advance(w, out)
        w['velocity'][0, :2] += f([[.5, -.2], [-.3, -.5]])
        out = hold(w)


def test_too_fast_for_the_lists_and_crawling(oracle):
    room = _box(0, 0, 4, 4) + _box(1.5, 1.5, 2, 2)
    w = world([room, room], [[[2.5, 1.]], [[2.5, 1.45]]], velocity=[[[20., -9.]], [[-6e-6, 0.]]])
    out = hold(w)
    assert (out['progress'] < 1).all()


def test_two_of_the_suites_plans_with_37_random_poses(oracle):
    from tests.rollout_rule import world_of
    c, _ = util.plan_world(2, 37, 8, 130, seed=3, device='cpu')
    w = world_of(c)
    rng = np.random.RandomState(2)
    w['velocity'] = rng.uniform(-3, 3, (2, 37, 2)).astype(f)
    w['angvelocity'] = rng.uniform(-90, 90, (2, 37)).astype(f)
    out = hold(w)
    assert (out['slid'] > 0).sum() > 5 and (out['progress'] >= 1).sum() > 5


def _crossings(walls, P, Q):
    """How many of the segments P[i] -> Q[i] cross a wall properly, in float64."""
    a, b = walls[:, None, :2].astype(float), walls[:, None, 2:].astype(float)
    P, Q = P[None].astype(float), Q[None].astype(float)
    cross = lambda u, v: u[..., 0]*v[..., 1] - u[..., 1]*v[..., 0]
    d1, d2 = cross(b - a, P - a), cross(b - a, Q - a)
    d3, d4 = cross(Q - P, a - P), cross(Q - P, b - P)
    return int(((d1*d2 < 0) & (d3*d4 < 0)).sum())


def _clearance(walls, P):
    a, b = walls[:, None, :2].astype(float), walls[:, None, 2:].astype(float)
    ab = b - a
    t = np.clip(((P[None] - a)*ab).sum(-1)/np.maximum((ab*ab).sum(-1), 1e-30), 0, 1)
    return float(np.sqrt((((P[None] - a - t[..., None]*ab))**2).sum(-1)).min())


@pytest.mark.parametrize('table,keep,seed', [(TABLE, 0., 5), (GENTLE, .875, 6)], ids=['simple', 'momentum'])
def test_no_step_crosses_a_wall(oracle, table, keep, seed):
    """Safety, in float64 and written apart from the rule: 64 walkers on two of the suite's closed plans, 300 steps of random
    actions. No centre segment p -> p1 or p1 -> p2 may cross a static wall - with the seeds chosen so that the plain step alone
    crosses none, the sliding step must cross none either. The least clearances are printed: a finding."""
    from tests.rollout_rule import world_of
    c, _ = util.plan_world(2, 32, 8, 130, seed=seed, device='cpu')
    base = world_of(c)
    rng = np.random.RandomState(seed)
    actions = rng.randint(0, 7, (300, 64, 1))
    start = dict(walls=[base['walls'][n] for n in (0, 1) for _ in range(32)],
                 **{k: base[k].reshape((64, 1) + base[k].shape[2:]).copy() for k in STATE})
    start['angles'] = rng.uniform(-180, 180, (64, 1)).astype(f)
    results = {}
    for slide in (False, True):
        w, crossings, least, slides = start, 0, np.inf, 0
        scene = plain_scene(w)
        for h in range(300):
            movement = (actions[h], table, keep)
            v, _ = _moved(w, movement)
            out = host_slide(w, RADIUS, FPS, .05, movement) if slide else plain_rule(w, RADIUS, FPS, movement, scene=scene)
            p = w['positions'].astype(float)
            p1 = p + out['progress'].astype(float)[..., None]*v.astype(float)/FPS
            for n in range(64):
                crossings += _crossings(w['walls'][n], p[n], p1[n]) + _crossings(w['walls'][n], p1[n], out['positions'][n])
                least = min(least, _clearance(w['walls'][n], out['positions'][n].astype(float)))
            slides += int((out['slid'] > 0).sum()) if slide else 0
            w = advance(w, out)
        results[slide] = crossings
        print(f'slide={slide}: {crossings} crossings, least clearance {least:.4f} m (R = {RADIUS}), {slides} slides')
        if slide:
            assert slides > 100
    assert results[False] == 0
    assert results[True] == 0


def test_arguments_are_refused(oracle):
    from megastep_amd import _lib
    w = world([LONG_WALL], [[[1., 1.]]])
    for bounce in (-.01, 1.01, float('nan')):
        assert host_slide(w, RADIUS, FPS, bounce, raw=True) == -1
    assert host_slide(w, RADIUS, FPS, 0., raw=True) == 0 and host_slide(w, RADIUS, FPS, 1., raw=True) == 0
    crowd = world([LONG_WALL], [np.stack([np.arange(65), np.ones(65)], -1)])
    assert host_slide(crowd, RADIUS, FPS, .05, raw=True) == -3
    h = _lib.lib()
    cfg = _lib.MsConfig(.1, 64, 130., 10.)
    assert h.ms_slide_physics(None, None, None, None, None, None, C.byref(cfg), None) == -1
    assert h.ms_slide_physics(C.byref(_lib.MsScenery()), C.byref(_lib.MsAgents()), None, None, C.byref(_lib.MsSlide(.05, None, None)), None,
                              C.byref(cfg), None) == -1
    assert h.ms_host_slide(None, None, 1, 1, None, None, None, None, None, C.byref(cfg)) == -1


@pytest.mark.parametrize('shape,others', [((7, 6), 'rest'), ((49, 4), 'rest'), ((7, 6), None)])
def test_rollouts_that_slide_are_a_loop_over_the_rule(oracle, shape, others):
    """ms_host_rollouts with slide on against a loop over the rule: two envs - a room with a pillar and two agents a step apart by
    its south wall, and a corridor - the other agents at rest (or absent), plans of actions that never turn."""
    from tests.slide_rule import ROLLOUT_FIELDS, host_rollouts_slide, rollout_slide_rule
    room = _box(0, 0, 4, 4) + _box(1.5, 1.5, 2, 2)
    w = world([room, _box(0, 0, 6, .5)], [[[1., .3], [1.3, .35]], [[1., .25], [3., .25]]], velocity=[[[1., -1.], [0., 0.]], [[2., .5], [-1., 0.]]])
    K, H = shape
    rng = np.random.RandomState(K)
    actions = rng.randint(-1, 6, (2, 2, K, H)) if K == 7 else rng.randint(0, 5, (K, H))
    want = rollout_slide_rule(w, actions, TABLE[:5], .875, others, RADIUS, FPS)
    got = host_rollouts_slide(w, actions, TABLE[:5], .875, others, RADIUS, FPS)
    for k in ROLLOUT_FIELDS:
        util.assert_bits(got[k], want[k], k)
    assert (want['slides'] > 0).any() and (want['stops'] > 0).any() and (want['stops'] == 0).any()


def test_rollout_arguments_are_refused(oracle):
    from tests.slide_rule import host_rollouts_slide
    w = world([LONG_WALL], [[[1., 1.]]])
    actions = np.zeros((3, 2), np.int64)
    assert host_rollouts_slide(w, actions, TABLE, 0., None, RADIUS, FPS, bounce=.05, raw=True) == 0
    for bounce in (-.01, 1.01, float('nan')):
        assert host_rollouts_slide(w, actions, TABLE, 0., None, RADIUS, FPS, bounce=bounce, raw=True) == -1
