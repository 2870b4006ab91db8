"""Walkers on the CPU: ms_host_walkers - walker_kernel's own __host__ __device__ pieces, swept serially - held to walk_rule in the
whole store and every record, floats by their bits; every refusal; and the rule against float64 geometry written apart from it."""
import numpy as np
import pytest

from tests import walker_rule as wr
from tests.walker_rule import F, KEYS, NAN, ROOM


def both(walls, agents, store, towards, ticks=1, **kw):
    """`ticks` calls in a row through the host statement and the rule, compared after each; the rule's result of every tick."""
    results = []
    for _ in range(ticks):
        got, want = wr.host_walk(walls, agents, store, towards, **kw), wr.walk_rule(walls, agents, store, towards, **kw)
        wr.same(got, want, KEYS)
        store = dict(store, **{k: want[k] for k in wr.STORE})
        results.append(want)
    return results


# slot: (position, velocity, target) - see test_the_box_room
WALKERS = [((.2, 2), (-1, 0), (-1, 2)), ((.2, .2), (-.7, -.7), (-1, -1)), ((2, 2), (1, 0), (3, 2)), ((2.35, 2), (-1, 0), (1, 2)),
           ((2, 3), (1, 0), (3, 3)), ((2.35, 3), (-1, 0), (1, 3)), ((2.7, 3), (-.5, 0), (1, 3)), ((6.1, .5), (1, 0), (7.5, .5)),
           ((6.05, 3.5), (0, 0), (NAN, 3.5)), ((1, 1), (0, 0), (1.03, 1)), ((3.5, .5), (NAN, 0), (5, .5)), ((NAN, NAN), (1, 1), (1, 1)),
           ((4.6, 2), (.6, -.6), (5.5, 1.5))]


@pytest.mark.parametrize('agents_push', [True, False])
@pytest.mark.parametrize('keep', [0., .9])
def test_the_box_room(keep, agents_push):
    """Slot 0 straight at a wall, 1 into a corner; 2 and 3 head-on; 4, 5, 6 in a row, the middle one walking at the first, the third behind
    it; 7 walking at agent 0, who is at rest; 8 on a NaN target inside `personal` of agent 1 without touching; 9 with a target nearer than a
    tick's step; 10 a NaN in its stored velocity; 11 empty; 12 into the partition.  Agent 2 is nowhere.  Env 1: the same, reset.  Six ticks."""
    store = wr.store(2, 13, [(n, k, p, v) for n in range(2) for k, (p, v, _) in enumerate(WALKERS)])
    store['speeds'][:, 6] = .5
    towards = np.array([[t for _, _, t in WALKERS]]*2, F)
    agents = np.array([[(6.5, .5), (6.5, 3.5), (NAN, 1)]]*2, F)
    ticks = both([ROOM, ROOM], agents, store, towards, ticks=6, keep=keep, agents_push=agents_push, reset=np.array([0, 1], np.uint8))
    first = ticks[0]
    assert list(first['blocked'][0, [0, 1, 2, 3, 5, 11]]) == [3, 3, 2, 2, 2, 4] and first['progress'][0, 4] != first['progress'][0, 6]
    assert (first['progress'][0, :4] < 1).all() and not first['velocities'][0, :4].any() and np.isnan(first['progress'][0, 11])
    assert list(first['close'][0]) == [1, 1, 0] and first['bumps'][0, 1] == 0 and any(t['bumps'][0, 0] == 1 and t['blocked'][0, 7] == 1 for t in ticks)
    moved = first['positions'][0] - store['positions'][0]
    assert (moved[8, 0] < 0) == agents_push and moved[8, 1] == 0                           # no target, and pushed all the same
    assert 0 < moved[9, 0] <= F(.03) + 1e-6 and (keep > 0 or abs(moved[9, 0] - .03) < 1e-6)  # never past its target
    assert not moved[10].any() and not first['velocities'][0, 10].any() and first['progress'][0, 10] == 1
    assert any(t['blocked'][0, 12] == 3 for t in ticks)
    assert all(np.isnan(t['positions'][1]).all() and (t['blocked'][1] == 4).all() and not t['bumps'][1].any() and not t['close'][1].any() for t in ticks)


REFUSALS = [[(k, None)] for k in ('positions', 'velocities', 'speeds', 'towards', 'agents', 'walls', 'starts')] + \
    [[(k, lambda p: p + 4)] for k in ('positions', 'velocities', 'towards', 'agents', 'walls')] + \
    [[(k, lambda p: p + 2)] for k in ('speeds', 'progress', 'bumps', 'close')] + \
    [[(k, v)] for k, vs in (('n_slots', (0, 1025)), ('n_agents', (0, 65)), ('n_envs', (0,)), ('personal', (0., np.inf, NAN)), ('push', (-1., np.inf, NAN)),
                            ('keep', (-.1, 1., NAN)), ('fps', (0., np.inf, NAN)), ('agent_radius', (0., np.inf, NAN)), ('agents_push', (2,))) for v in vs]


@pytest.mark.parametrize('spoil', REFUSALS, ids=lambda s: '-'.join(f'{k}-{v}' if isinstance(v, (int, float)) else k for k, v in s))
def test_the_argument_check_refuses(spoil):
    args = ([ROOM], np.ones((1, 2, 2), F), wr.store(1, 4), np.ones((1, 4, 2), F))
    wr.host_walk(*args, expect=-1, spoil=spoil)
    wr.host_walk(*args)


@pytest.mark.parametrize('n', [1, 4])
def test_no_step_crosses_a_wall_in_float64(n):
    """Sixteen walkers from free cells of an axis-aligned and of an oblique plan, 64 ticks towards the waypoints of one goal round an agent
    at rest, host statement == rule at every tick: no step crosses a static wall. Overlap is not asserted: the deepest is printed."""
    from tests.test_navfield_host import RADIUS, _crossings
    from tests.test_navpath_host import cases, path_rule
    case = cases()[n]
    starts = case.points[np.isfinite(case.g)][:17]
    walls, agents, store = [case.walls.reshape(-1, 4)], starts[None, :1], wr.store(1, 16, [(0, k, p, (0, 0)) for k, p in enumerate(starts[1:])])
    store['speeds'][:] = np.linspace(.6, 1.4, 16, dtype=F)
    steps, deepest = [], np.inf
    for _ in range(64):
        towards = np.array([[path_rule.waypoint(case.world, p, 16, case.table)[0] for p in store['positions'][0]]], F)
        out = wr.walk_rule(walls, agents, store, towards, radius=RADIUS, steps=steps)
        wr.same(wr.host_walk(walls, agents, store, towards, radius=RADIUS), out, KEYS)
        store = dict(store, **{k: out[k] for k in wr.STORE})
        p = out['positions'][0].astype(np.float64)
        deepest = min(deepest, (np.linalg.norm(p[:, None] - p[None], axis=-1) + 9*np.eye(16)).min() - 2*RADIUS)
    steps = np.array(steps, np.float64)
    walked = np.linalg.norm(steps[:, 2:] - steps[:, :2], axis=1)
    print(f'plan {n}: {len(steps)} steps, {walked.sum():.1f} m walked, the least gap between two walkers {deepest:.4f} m')
    assert len(steps) == 64*16 and walked.sum() > 30
    assert _crossings(steps[:, :2], steps[:, 2:], case.walls) == 0
