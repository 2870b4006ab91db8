"""Sliding walkers on the CPU: ms_host_walkers with slide - walker_slide_kernel's own __host__ __device__ pieces, swept serially -
held to walk_slide_rule in the whole store and every record, floats by their bits; the plain call where nobody is blocked; the cure
against float64 geometry written apart from the rule; the refusals."""
import numpy as np
import pytest

from tests import walker_rule as wr
from tests import walker_slide_rule as ws
from tests.test_walker_host import WALKERS
from tests.walker_rule import F, NAN, ROOM

# test_the_box_room's slots, then: 13 obliquely into the wall x = 0; 14 up into the wall y = 4 and along it into 15, which stands
SLOTS = WALKERS + [((.4, 3), (-.8, .6), (-2, 4.8)), ((3, 3.7), (.7, .7), (6, 6.7)), ((3.6, 3.8), (0, 0), (NAN, NAN))]


@pytest.mark.parametrize('bounce', [0., .05])
@pytest.mark.parametrize('keep', [0., .9])
def test_the_box_room_sliding(keep, bounce):
    """Slot 0 head-on at a wall (its deflected move is purely normal: it stays at p1), 1 into a corner (phase B blocked at once), 2 and 3
    head-on, 7 at an agent at rest, 8 a NaN target, 11 empty, 12 head-on into the partition, 13 obliquely into a wall (slides), 14 along a
    wall into where 15's phase A left it (slides, then stopped).  Env 1: the same, reset.  Six ticks, host statement == rule as bits."""
    store = wr.store(2, len(SLOTS), [(n, k, p, v) for n in range(2) for k, (p, v, _) in enumerate(SLOTS)])
    towards = np.array([[t for _, _, t in SLOTS]]*2, F)
    agents = np.array([[(6.5, .5), (6.5, 3.5), (NAN, 1)]]*2, F)
    kw = dict(keep=keep, bounce=bounce, personal=.35, reset=np.array([0, 1], np.uint8))
    ticks = []
    for _ in range(6):
        want = ws.walk_slide_rule([ROOM, ROOM], agents, store, towards, **kw)
        wr.same(ws.host_walk_slide([ROOM, ROOM], agents, store, towards, **kw), want, ws.KEYS)
        plain = wr.walk_rule([ROOM, ROOM], agents, store, towards, **{k: v for k, v in kw.items() if k != 'bounce'})
        wr.same(want, plain, wr.KEYS[2:])                                # phase A's records are the plain tick's
        store = dict(store, **{k: want[k] for k in wr.STORE})
        ticks.append(want)
    rec = {k: np.stack([t[k][0] for t in ticks]) for k in ws.KEYS}       # (tick, slot) of env 0
    slid, dead, x1 = rec['slid'], rec['stopped'] == 1, rec['progress']
    assert ((slid[:, 13] > 0) & ~dead[:, 13] & (rec['blocked'][:, 13] == 3)).any()
    assert (dead[:, 1] & (x1[:, 1] < 1) & (slid[:, 1] < 1 - x1[:, 1])).any()
    assert ((slid[:, 14] > 0) & dead[:, 14]).any() and (rec['blocked'][:, 14] == 3).any()
    assert (rec['blocked'][:, [2, 3]] == 2).any() and (rec['blocked'][:, 7] == 1).any() and (rec['blocked'][:, 0] == 3).any()
    assert bounce > 0 or (rec['positions'][:, 0, 1] == 2).all()           # head-on: nowhere to slide to
    assert (rec['stopped'][:, 11] == 4).all() and np.isnan(slid[:, 11]).all() and not np.ptp(rec['positions'][:, 8], 0).any()
    assert all(np.isnan(t['slid'][1]).all() and (t['stopped'][1] == 4).all() and np.isnan(t['positions'][1]).all() for t in ticks)


def test_nobody_blocked_is_the_plain_call():
    """An open world - no rows, the bodies metres apart: every output of the sliding call is the plain call's, slid 0 where present."""
    store, towards = wr.random_store(2, 12, [np.zeros(2)]*2, [np.full(2, 40.)]*2, 5)
    store['positions'] += (np.arange(12, dtype=F)*9)[None, :, None]       # (the cluster pulled apart)
    agents, walls = np.full((2, 2, 2), -9, F), [np.zeros((0, 4), F)]*2
    plain, sliding = wr.host_walk(walls, agents, store, towards), ws.host_walk_slide(walls, agents, store, towards)
    wr.same(sliding, plain, wr.KEYS)
    there = np.isfinite(store['positions']).all(-1)
    assert there.any() and (plain['progress'][there] == 1).all() and (plain['velocities'][there] != 0).any()
    assert (sliding['slid'][there] == 0).all() and (sliding['stopped'][there] == 0).all() and np.isnan(sliding['slid'][~there]).all()


def test_a_walker_steered_at_45_degrees_into_a_wall_slides_along_it():
    """keep = 0, towards the wall y = 0 at 45 degrees, 1 m/s: plainly its displacement along the wall is 0 once it touches (from the
    fourth tick on: the second closes the gap, the third what the contact test's margin left); sliding it goes on along the wall at more
    than half of cos(45 deg)/fps a tick, at a radius from it."""
    store, towards = wr.store(1, 1, [(0, 0, (2, .2), (0, 0))]), np.array([[(6, -3.8)]], F)
    along = {}
    for slide in (0, 1):
        s, moved = store, []
        for _ in range(6):
            out = ws.host_walk_slide([ROOM], np.full((1, 1, 2), NAN, F), s, towards, keep=0., slide=slide)
            moved.append((out['positions'][0, 0, 0] - s['positions'][0, 0, 0], out['progress'][0, 0], out['slid'][0, 0] if slide else 0))
            s = dict(s, **{k: out[k] for k in wr.STORE})
        along[slide] = np.array(moved, np.float64)
    touching = along[0][:, 1] < 1
    assert touching[1:].all() and (along[0][3:, 0] == 0).all()
    assert (along[1][1:, 2] > 0).all() and (along[1][1:, 0] > .035).all() and abs(s['positions'][0, 0, 1] - wr.RADIUS) < .01


@pytest.mark.parametrize('n', [1, 4])
def test_no_sliding_step_crosses_a_wall_in_float64(n):
    """test_no_step_crosses_a_wall_in_float64's walk with slide: neither a phase-A nor a phase-B segment crosses a static wall."""
    from tests.test_navfield_host import RADIUS, _crossings
    from tests.test_navpath_host import cases, path_rule
    case = cases()[n]
    starts = case.points[np.isfinite(case.g)][:17]
    walls, agents, store = [case.walls.reshape(-1, 4)], starts[None, :1], wr.store(1, 16, [(0, k, p, (0, 0)) for k, p in enumerate(starts[1:])])
    store['speeds'][:] = np.linspace(.6, 1.4, 16, dtype=F)
    steps, slides = [], 0
    for _ in range(64):
        towards = np.array([[path_rule.waypoint(case.world, p, 16, case.table)[0] for p in store['positions'][0]]], F)
        out = ws.walk_slide_rule(walls, agents, store, towards, radius=RADIUS, steps=steps)
        wr.same(ws.host_walk_slide(walls, agents, store, towards, radius=RADIUS), out, ws.KEYS)
        store, slides = dict(store, **{k: out[k] for k in wr.STORE}), slides + int((out['slid'] > 0).sum())
    steps = np.array(steps, np.float64)
    print(f'plan {n}: {slides} slides in {len(steps)//2} steps, {np.linalg.norm(steps[:, 2:] - steps[:, :2], axis=1).sum():.1f} m walked')
    assert len(steps) == 2*64*16 and slides > 0
    assert _crossings(steps[:, :2], steps[:, 2:], case.walls) == 0


@pytest.mark.parametrize('spoil,expect', [(('slide', 2), -1), (('bounce', -.1), -1), (('bounce', 1.5), -1), (('bounce', NAN), -1),
                                          (('slid', lambda p: p + 2), -1), (('slid', None), 0), (('stopped', None), 0)])
def test_the_argument_check_refuses(spoil, expect):
    args = ([ROOM], np.ones((1, 2, 2), F), wr.store(1, 4), np.ones((1, 4, 2), F))
    ws.host_walk_slide(*args, expect=expect, spoil=[spoil])
    wr.host_walk(*args, spoil=[('bounce', -7.), ('slid', 2), ('stopped', 1)])     # (slide = 0: none of them is read)
