"""Items on the CPU: the host instantiations ms_host_item_collect and ms_host_item_overlay - kernels/items.h's own __host__
__device__ functions swept serially - held to EQUALITY with tests/item_rule.py's numpy rule, floats as bits, on the six plans and
on hand-made worlds; the overlay pinned to the fold that exists and held against float64 geometry written apart from the rule; the
header, the mirrors, every refusal, and the Python layer's arithmetic and refusals. No kernel is launched here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import item_rule as ir
from tests.item_rule import COLLECT_KEYS, F, INF, NAN, OVERLAY_KEYS, item_rule
from tests.test_navview_host import box_walls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOX = [box_walls()]


def _both_collect(walls, agents, positions, timers, kinds, K, reach, **kw):
    got = ir.host_collect(walls, agents, positions, timers, kinds, K, reach, **kw)
    want = item_rule.collect(walls, agents, positions, timers, kinds, K, reach, **kw)
    ir.same(got, want, COLLECT_KEYS)
    return want


def _one(agents, items, reach, timers=None, kinds=None, K=1, walls=BOX, **kw):
    """One env: agents (A, 2), items (P, 2)."""
    agents, items = np.asarray(agents, F)[None], np.asarray(items, F)[None]
    P = items.shape[1]
    timers = np.zeros((1, P), np.int32) if timers is None else np.asarray(timers, np.int32)[None]
    kinds = np.zeros((1, P), np.int32) if kinds is None else np.asarray(kinds, np.int32)[None]
    return _both_collect(walls, agents, items, timers, kinds, K, reach, **kw)


# ---------------------------------------------------------------------------------------------------------------------
# collect
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('A', [1, 4, 64])
@pytest.mark.parametrize('P', [1, 63, 64, 65, 1024])
def test_the_collect_is_the_rule_on_the_hand_made_world(P, A):
    w = ir.hand_items(P, A)
    taken = 0
    for through in (False, True):
        for takers in (None, w.takers):
            want = _both_collect(w.walls, w.agents, w.positions, w.timers, w.kinds, 8, .35, delay=3, takers=takers, through_walls=through)
            taken += int((want['taker'] >= 0).sum())
    assert taken > 0 or P == 1


def test_the_collect_is_the_rule_on_the_six_plans():
    w = ir.plan_items()
    blocked = _both_collect(w.walls, w.agents, w.positions, w.timers, w.kinds, 3, .5, delay=2)
    through = _both_collect(w.walls, w.agents, w.positions, w.timers, w.kinds, 3, .5, delay=2, through_walls=True)
    n_blocked, n_through = int((blocked['taker'] >= 0).sum()), int((through['taker'] >= 0).sum())
    assert 20 < n_blocked < n_through                                   # (the walls do stop some; the equality means something)
    assert blocked['counts'].sum() == n_blocked and (blocked['counts'].sum((0, 1)) > 0).all()
    # a kind outside [0, K) is taken and counted nowhere
    fewer = _both_collect(w.walls, w.agents, w.positions, w.timers, w.kinds, 2, .5)
    assert int((fewer['taker'] >= 0).sum()) == n_blocked and fewer['counts'].sum() < n_blocked


def test_equal_distances_go_to_the_lower_index_and_the_bound_is_closed():
    want = _one([(1.75, 2), (2.25, 2)], [(2, 2)], .5)
    assert want['taker'][0, 0] == 0
    want = _one([(3, 3), (2.25, 2), (1.75, 2)], [(2, 2)], .5)
    assert want['taker'][0, 0] == 1
    # (3, 4) scaled by an eighth: rr = .390625 = .625^2 exactly
    at = _one([(1, 1)], [(1.375, 1.5)], .625)
    assert at['taker'][0, 0] == 0 and at['due'][0, 0] == 1 and np.isnan(at['positions'][0, 0]).all()
    beyond = _one([(1, 1)], [(1.375, 1.5)], float(np.nextafter(F(.625), F(0))))
    assert beyond['taker'][0, 0] == -1 and beyond['due'][0, 0] == 0 and np.array_equal(beyond['positions'][0, 0], F([1.375, 1.5]))


def test_walls_block_a_taker_unless_told_otherwise():
    # the partition at x = 4 stands from y = 0 to 1.5 and from 2.5 to 4; its door is between
    behind = _one([(3.9, 1)], [(4.1, 1)], .25)
    assert behind['taker'][0, 0] == -1
    assert _one([(3.9, 1)], [(4.1, 1)], .25, through_walls=True)['taker'][0, 0] == 0
    assert _one([(3.9, 2)], [(4.1, 2)], .25)['taker'][0, 0] == 0                          # (through the door)
    # the nearer agent is behind the wall: the farther one takes
    assert _one([(3.95, 1), (4.3, 1)], [(4.1, 1)], .25)['taker'][0, 0] == 1
    # an item on the vertex two walls share: neither has it on one side, nothing blocks
    for agent in ((7.8, .2), (7.9, .05)):
        assert _one([agent], [(8, 0)], .5)['taker'][0, 0] == 0
    corner = [np.array([(1, 2, 2, 2), (2, 2, 2, 3)], F)]
    for agent in ((2.2, 1.8), (1.8, 2.2), (1.8, 1.8), (2.2, 2.2)):
        assert _one([agent], [(2, 2)], .5, walls=corner)['taker'][0, 0] == 0


def test_agents_that_are_nowhere_masked_takers_and_reset():
    w = ir.hand_items(65, 4)
    agents = w.agents.copy()
    agents[0, 1] = (NAN, 1.)
    agents[0, 2] = (INF, 1.)
    want = _both_collect(w.walls, agents, w.positions, w.timers, w.kinds, 8, .5)
    assert not np.isin(want['taker'], (1, 2)).any() and (want['taker'] >= 0).any()
    none = _both_collect(w.walls, w.agents, w.positions, w.timers, w.kinds, 8, .5, takers=np.zeros((1, 4), np.uint8))
    assert (none['taker'] == -1).all() and none['counts'].sum() == 0
    # reset: two envs, one emptied
    two = [np.concatenate([a, a]) for a in (w.agents, w.positions, w.timers, w.kinds)]
    want = _both_collect(w.walls*2, *two, 8, .5, delay=5, reset=np.array([0, 1], np.uint8))
    assert np.isnan(want['positions'][1]).all() and (want['timers'][1] == 0).all() and (want['due'][1] == 1).all()
    assert (want['taker'][1] == -1).all() and want['counts'][1].sum() == 0 and (want['taker'][0] >= 0).any()


@pytest.mark.parametrize('delay', [0, 1, -1])
def test_timers_and_due_over_a_sequence_of_calls(delay):
    """Eight calls with a return step between them: a due item with an even number comes back next to an agent, one with an odd
    number finds no cell and stays (NaN, NaN) with timer 0 - due again at the next call."""
    w = ir.hand_items(64, 4)
    host = dict(positions=w.positions.copy(), timers=w.timers.copy())
    rule = dict(positions=w.positions.copy(), timers=w.timers.copy())
    rng = np.random.RandomState(3)
    seen_due = stayed = taken = 0
    before = None
    for step in range(8):
        got = ir.host_collect(w.walls, w.agents, host['positions'], host['timers'], w.kinds, 8, .35, delay=delay)
        want = item_rule.collect(w.walls, w.agents, rule['positions'], rule['timers'], w.kinds, 8, .35, delay=delay)
        ir.same(got, want, COLLECT_KEYS)
        took = want['taker'] >= 0
        taken += int(took.sum())
        if delay == 0:
            assert (want['due'][took] == 1).all()
        if delay == 1 and before is not None:
            assert (want['due'][before] == 1).all()                     # (taken at the last call: due at this one)
        if delay != 0:
            assert (want['due'][took] == 0).all()
        if delay == -1:
            assert (want['timers'][took] == -1).all()
        if before is not None:
            stayed += int((want['due'][0, 1::2] & due_before[0, 1::2]).sum())
        before, due_before = took, want['due'].copy()
        seen_due += int(want['due'].sum())
        back = (want['due'] == 1) & (np.arange(64)[None] % 2 == 0)
        spots = (w.agents[0, rng.randint(0, 4, 64)] + rng.uniform(-.3, .3, (64, 2))).astype(F)[None]
        for store, out in ((host, got), (rule, want)):
            store['positions'] = np.where(back[..., None], spots, out['positions'])
            store['timers'] = out['timers']
    assert taken > 8 and seen_due > 0 and stayed > 0


# ---------------------------------------------------------------------------------------------------------------------
# overlay
# ---------------------------------------------------------------------------------------------------------------------
def _both_overlay(positions, colors, origins, dirs, radius, near, widths, planes, **kw):
    got = ir.host_overlay(positions, colors, origins, dirs, radius, near, widths, planes, **kw)
    want = item_rule.overlay(positions, colors, origins, dirs, radius, near, widths, planes)
    ir.same(got, want, [k for k in OVERLAY_KEYS if k in got])
    return want


def _hand_rays(w, per):
    """A ring of `per` rays from each agent of a hand-made world, and the planes the box's walls leave under them."""
    A = w.agents.shape[1]
    dirs = np.concatenate([ir.ring(per, phase=.37*a) for a in range(A)])[None]
    return dirs, ir.wall_planes(w.walls, w.agents, dirs, .1, w.widths, 2*A)


@pytest.mark.parametrize('P', [1, 64, 65, 256])
@pytest.mark.parametrize('per', [1, 37, 64, 65, 200])
def test_the_overlay_is_the_rule_on_the_hand_made_world(per, P):
    w = ir.hand_items(P, 3)
    dirs, base = _hand_rays(w, per)
    want = _both_overlay(w.positions, w.colors, w.agents, dirs, .1, .1, w.widths, base)
    if per >= 37 and P >= 64:
        shown = want['items'] >= 0
        assert shown.any() and not shown.all()
        absent = np.flatnonzero(np.isnan(w.positions[0, :, 0]))
        assert len(absent) and not np.isin(want['items'], absent).any()                  # (absent items in the middle of the store)
        assert (want['indices'][shown] == w.widths[0] + want['items'][shown]).all()
        assert np.array_equal(ir.bits(want['distances'][~shown]), ir.bits(base['distances'][~shown]))
    # the rays as a cast's: an origin a ray
    each = np.repeat(w.agents, per, 1)
    again = _both_overlay(w.positions, w.colors, each, dirs, .1, .1, w.widths, base)
    ir.same(again, want, OVERLAY_KEYS)


@pytest.mark.parametrize('P', [257, 512, 1023, 1024])
@pytest.mark.parametrize('per', [255, 256, 257, 600])
def test_the_wide_item_sets_hold_what_they_are_named_for(per, P):
    """The sets tests/test_gpu_items.py puts item_overlay_kernel's second window and second chunk through: their counts, window by
    window, and - over the box's walls as the numpy cast leaves them - rays of every origin and of the last chunk that show an item."""
    w0 = ir.hand_items(P, 3)
    dirs, base = _hand_rays(w0, per)
    chunks = -(-per//ir.OVERLAY_WINDOW)
    for which in ir.WIDE_SETS:
        w = ir.wide_items(P, which)
        ir.check_wide(w, which)
        got = ir.host_overlay(w.positions, w.colors, w.agents, dirs, ir.WIDE_RADIUS, .1, w.widths, base)
        shown = (got['items'] >= 0).reshape(3, per)
        assert shown.any() and not shown.all(), which
        assert shown[:, (chunks - 1)*ir.OVERLAY_WINDOW:].any() or (which, P) == ('late', 257), which     # ('late', 257): one item in all


@pytest.mark.parametrize('P', [257, 512, 1023, 1024])
@pytest.mark.parametrize('per', [257, 600])
def test_the_overlay_is_the_rule_on_the_wide_item_sets(per, P):
    w0 = ir.hand_items(P, 3)
    dirs, base = _hand_rays(w0, per)
    for which in ir.WIDE_SETS:
        w = ir.wide_items(P, which)
        want = _both_overlay(w.positions, w.colors, w.agents, dirs, ir.WIDE_RADIUS, .1, w.widths, base)
        if which == 'on':                                                # (the item under an origin is never what that origin sees)
            assert not (want['items'].reshape(3, per)[0] == 1).any() and not (want['items'].reshape(3, per)[1] == ir.OVERLAY_WINDOW).any()


def test_the_overlay_is_the_rule_on_the_six_plans():
    w = ir.plan_items()
    base = ir.wall_planes(w.walls, w.agents, w.dirs, .1, w.widths, 6)
    want = _both_overlay(w.positions, w.colors, w.agents, w.dirs, .1, .1, w.widths, base)
    assert 200 < (want['items'] >= 0).sum() < want['items'].size - 200


def _line(items, base_distance, near=.125, radius=.125, origin=(1, 2), ru=(1, 0), **kw):
    """One ray from `origin` along `ru` over the items given, the plane holding `base_distance`; returns the rule's planes."""
    positions = np.asarray(items, F)[None]
    P = positions.shape[1]
    colors = np.linspace(.2, 1, 3*P).astype(F).reshape(1, P, 3)
    planes = dict(distances=np.array([[base_distance]], F), indices=np.array([[7 if np.isfinite(base_distance) else -1]], np.int32),
                  locations=np.array([[.5]], F), dots=np.array([[.1]], F), screen=np.full((1, 1, 3), .25, F))
    return _both_overlay(positions, colors, np.asarray([[origin]], F), np.asarray([[ru]], F), radius, near, [10], planes, **kw)


def test_the_near_plane_walls_bodies_and_a_missed_ray():
    # an item exactly at the near plane is not drawn (near < s is strict); a step beyond it is
    assert _line([(1.125, 2)], 5.)['items'][0, 0] == -1
    shown = _line([(1.25, 2)], 5.)
    assert shown['items'][0, 0] == 0 and shown['distances'][0, 0] == F(.25) and shown['indices'][0, 0] == 10
    # a ray of another length: d = s |ru| is the same distance
    assert _line([(1.25, 2)], 5., ru=(2, 0))['distances'][0, 0] == F(.25)
    # in front of a wall (or a body: whatever the plane holds) the item replaces the ray; behind it, or exactly as far, it does not
    front = _line([(3, 2)], 2.5)
    assert front['items'][0, 0] == 0 and front['distances'][0, 0] == 2 and front['dots'][0, 0] == 0 and front['locations'][0, 0] == F(.5)
    assert np.array_equal(front['screen'][0, 0], np.linspace(.2, 1, 3).astype(F))       # (seen square on: dn = 1, the item's own colour)
    for held in (1.5, 2.):
        behind = _line([(3, 2)], held)
        assert behind['items'][0, 0] == -1 and behind['distances'][0, 0] == F(held) and behind['indices'][0, 0] == 7
        assert (behind['screen'] == F(.25)).all() and behind['dots'][0, 0] == F(.1)
    # a missed ray holds +inf: any item on it is drawn
    missed = _line([(3, 2)], np.inf)
    assert missed['items'][0, 0] == 0 and missed['distances'][0, 0] == 2
    # an origin on an item: a NaN row, never hit - the item behind it is seen
    on = _line([(1, 2), (3, 2)], 5.)
    assert on['items'][0, 0] == 1
    assert _line([(1, 2)], 5.)['items'][0, 0] == -1
    # an item off the ray by more than its radius is missed, by less it is hit off its centre
    assert _line([(3, 2.13)], 5.)['items'][0, 0] == -1
    grazed = _line([(3, 2.12)], 5.)
    assert grazed['items'][0, 0] == 0 and grazed['locations'][0, 0] < .05 and 0 < abs(grazed['dots'][0, 0]) < .1


def test_two_items_in_line_and_the_folds_hysteresis():
    # met in ascending k: a later item must be nearer by more than 1e-4 in s to take the ray
    inside = _line([(3.00005, 2), (3, 2)], 5.)
    assert inside['items'][0, 0] == 0 and inside['distances'][0, 0] > 2
    outside = _line([(3.001, 2), (3, 2)], 5.)
    assert outside['items'][0, 0] == 1 and outside['distances'][0, 0] == 2
    assert _line([(3, 2), (3.00005, 2)], 5.)['items'][0, 0] == 0
    assert _line([(3, 2), (4, 2)], 5.)['items'][0, 0] == 0 and _line([(4, 2), (3, 2)], 5.)['items'][0, 0] == 1


def test_every_optional_plane_may_be_null():
    w = ir.hand_items(65, 3)
    dirs, base = _hand_rays(w, 37)
    full = _both_overlay(w.positions, w.colors, w.agents, dirs, .1, .1, w.widths, base)
    for leave in ('indices', 'locations', 'dots', 'screen', 'items'):
        planes = {k: v for k, v in base.items() if k != leave}
        got = ir.host_overlay(w.positions, w.colors, w.agents, dirs, .1, .1, None if leave == 'indices' else w.widths, planes,
                              items=leave != 'items')
        assert leave not in got
        ir.same(got, full, [k for k in OVERLAY_KEYS if k != leave])
    bare = ir.host_overlay(w.positions, None, w.agents, dirs, .1, .1, None, dict(distances=base['distances']), items=False)
    ir.same(bare, full, ['distances'])


def test_an_agents_body_hides_the_item_behind_it_and_not_the_one_in_front():
    """The planes of a cast that met a body: a small square round agent 1, as its model's rows would stand."""
    w = ir.hand_items(1, 2)
    agents = np.array([[(1, 2), (3, 2)]], F)
    body = np.array([(2.9, 1.9, 2.9, 2.1), (2.9, 2.1, 3.1, 2.1), (3.1, 2.1, 3.1, 1.9), (3.1, 1.9, 2.9, 1.9)], F)
    dirs = np.concatenate([ir.fan(0., 33, 40.), ir.fan(np.pi, 33, 40.)])[None]
    base = ir.wall_planes([np.concatenate([body, box_walls()])], agents, dirs, .1, [8 + len(box_walls())], 0)
    centre = 16                                                          # (agent 0's ray straight at agent 1)
    assert abs(base['distances'][0, centre] - 1.9) < 1e-5
    for x, shows in ((2.5, True), (3.5, False)):
        positions = np.array([[(x, 2)]], F)
        want = _both_overlay(positions, w.colors, agents, dirs, .1, .1, [14], base)
        assert (want['items'][0, centre] == 0) == shows


def test_the_overlay_agrees_with_the_fold_that_exists_on_a_wall_that_is_the_billboard():
    """An env gains one extra static wall equal to an item's billboard for one origin; the planes of a cast on it (the numpy
    restatement of the reference's fold over walls: no host instantiation of the raycast exists) against the overlay on the env
    without that wall. Where the billboard beats every other hit by more than 1e-3 in s, distance, location and dot agree as bits."""
    w = ir.plan_items()
    agree = 0
    for n in range(6):
        origin = w.agents[n, :1]
        for k in np.flatnonzero(np.isfinite(w.positions[n, :, 0]))[:12]:
            c = w.positions[n, k]
            row = np.array([float(v) for v in ir.billboard(origin[0, 0], origin[0, 1], c[0], c[1], .1)], F)
            if not np.isfinite(row).all():
                continue
            towards = float(np.arctan2(c[1] - origin[0, 1], c[0] - origin[0, 0]))
            dirs = ir.fan(towards, 65, 12.)[None]
            plain = ir.raycast([w.walls[n]], origin[None], dirs, .1)
            walled = ir.raycast([np.concatenate([w.walls[n], row[None]])], origin[None], dirs, .1)
            over = ir.host_overlay(c[None, None], None, origin[None], dirs, .1, .1, None, {k_: plain[k_] for k_ in ('distances', 'locations', 'dots')})
            with np.errstate(all='ignore'):
                s_plain = plain['distances'][0]/ir.ray_lengths(dirs[0])[2]
                s_wall = walled['distances'][0]/ir.ray_lengths(dirs[0])[2]
            clear = (walled['indices'][0] == len(w.walls[n])) & (s_plain - s_wall > 1e-3)
            assert (over['items'][0][clear] == 0).all()
            for key in ('distances', 'locations', 'dots'):
                assert np.array_equal(ir.bits(over[key][0][clear]), ir.bits(walled[key][0][clear])), (n, k, key)
            agree += int(clear.sum())
    assert agree > 300


def _float64_scene(w, n):
    """Per ray of env n of plan_items(), in float64 and written apart from the rule: the distance to the nearest wall crossing, and
    per item the distance at which the ray crosses the item's diameter square to the line of sight and how far from the centre."""
    A = w.agents.shape[1]
    per = w.dirs.shape[1]//A
    p = np.repeat(w.agents[n].astype(np.float64), per, 0)                  # (R, 2)
    u = w.dirs[n].astype(np.float64)
    u = u/np.linalg.norm(u, axis=1, keepdims=True)
    walls = w.walls[n].astype(np.float64)
    a, v = walls[:, :2], walls[:, 2:] - walls[:, :2]
    q = a[None] - p[:, None]                                               # (R, L, 2)
    denom = u[:, None, 0]*v[None, :, 1] - u[:, None, 1]*v[None, :, 0]
    with np.errstate(all='ignore'):
        s = (q[..., 0]*v[None, :, 1] - q[..., 1]*v[None, :, 0])/denom
        t = (q[..., 0]*u[:, None, 1] - q[..., 1]*u[:, None, 0])/denom
    s = np.where((np.abs(denom) > 1e-9) & (t >= 0) & (t <= 1) & (s > .1), s, np.inf)
    wall = s.min(1)
    c = w.positions[n].astype(np.float64)
    to = c[None] - p[:, None]                                              # (R, P, 2)
    dist = np.linalg.norm(to, axis=-1)
    along = (to*u[:, None]).sum(-1)
    with np.errstate(all='ignore'):
        cross = dist*dist/along                                            # (the ray meets the line through c square to p -> c here)
        hit = p[:, None] + cross[..., None]*u[:, None]
        off = np.linalg.norm(hit - c[None], axis=-1)
    cross = np.where(along > 0, cross, np.inf)
    return wall, cross, off


#: the largest deviation of the rule's d from the float64 crossing on the six plans, as measured
D_DEVIATION = 8.5e-7


def test_the_rule_against_float64_geometry_on_the_six_plans():
    """No item is drawn through a wall, none in plain sight is missing - outside a band at the billboard's ends and at the wall's
    distance - and the rule's d stays within four times its own measured deviation from the float64 crossing."""
    w = ir.plan_items()
    base = ir.wall_planes(w.walls, w.agents, w.dirs, .1, w.widths, 6)
    rule = item_rule.overlay(w.positions, w.colors, w.agents, w.dirs, .1, .1, w.widths, base)
    band, worst, through, missing, drawn, plain = 1e-3, 0., 0, 0, 0, 0
    for n in range(6):
        wall, cross, off = _float64_scene(w, n)
        k = rule['items'][n]
        shown = np.flatnonzero(k >= 0)
        drawn += len(shown)
        through += int((cross[shown, k[shown]] > wall[shown] + band).sum())
        worst = max(worst, float(np.abs(rule['distances'][n][shown].astype(np.float64) - cross[shown, k[shown]]).max()))
        with np.errstate(invalid='ignore'):
            sure = (off <= .1*(1 - band)) & (cross > .1 + band) & (cross < wall[:, None] - band)
        first = np.where(sure, cross, np.inf).min(1)
        rays = np.flatnonzero(np.isfinite(first))
        plain += len(rays)
        missing += int(((k[rays] < 0) | (rule['distances'][n][rays] > first[rays] + 2e-4)).sum())
    print(f'rays with an item drawn {drawn}, with one in plain sight {plain}; the largest deviation of d {worst:.3g}')
    assert drawn > 200 and plain > 200 and through == 0 and missing == 0
    assert worst <= 4*D_DEVIATION


# ---------------------------------------------------------------------------------------------------------------------
# the header, the mirrors, the refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_the_headers_declare_the_calls_and_the_abi_version_stays():
    from megastep_amd import _lib
    text = open(os.path.join(ROOT, 'include', 'megastep_hip.h')).read()
    assert re.search(r'#define MS_ABI_VERSION 17\b', text) and _lib.ABI_VERSION == 17
    assert re.search(r'int ms_item_collect\(const MsScenery\* \w+, const MsAgents\* \w+, const MsItemCollect\* \w+, void\* \w+\);', text)
    assert re.search(r'int ms_item_overlay\(const MsScenery\* \w+, const MsItemOverlay\* \w+, void\* \w+\);', text)
    hooks = open(os.path.join(ROOT, 'include', 'megastep_hip_test.h')).read()
    assert 'int ms_host_item_collect(' in hooks and 'int ms_host_item_overlay(' in hooks
    for struct, fields in (('MsItemCollect', 'n_items n_kinds positions timers kinds takers reset reach delay through_walls taker counts due'),
                           ('MsItemOverlay', 'n_items n_rays n_origins positions colors origins dirs radius near_plane distances indices '
                                             'locations dots screen items')):
        body = re.search(r'typedef struct %s \{(.*?)\} %s;' % (struct, struct), text, flags=re.S).group(1)
        body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
        assert re.findall(r'(\w+);', body) == fields.split() == [f for f, _ in getattr(_lib, struct)._fields_]


def test_bad_arguments_are_refused_before_any_launch():
    """Every refusal the header lists, through the host instantiations (which share the launches' checks) and, with NULL structs,
    through the launches themselves. Host memory stands in for the device's: nothing here gets as far as a kernel."""
    from megastep_amd import _lib
    h = _lib.lib()
    buf = np.zeros(256, np.float32)
    base = buf.ctypes.data + (-buf.ctypes.data) % 16
    p, odd8, odd4 = base, base + 4, base + 2
    starts = np.zeros(2, np.int64)

    def collect(n_envs=1, n_agents=1, agents=p, walls=p, wall_starts=starts.ctypes.data, **kw):
        spec = dict(n_items=1, n_kinds=1, positions=p, timers=p, kinds=p, reach=1., delay=0, through_walls=1, taker=None, counts=None, due=None)
        spec.update(kw)
        return h.ms_host_item_collect(C.byref(_lib.MsItemCollect(**spec)), n_envs, n_agents, agents, walls, wall_starts)

    buf[:2] = np.nan                                                     # (the one item is absent; timers and kinds read it as ints)
    assert collect() == 0
    bad = [dict(n_items=0), dict(n_items=1025), dict(n_kinds=0), dict(n_kinds=9), dict(positions=None), dict(timers=None), dict(kinds=None),
           dict(reach=0.), dict(reach=-1.), dict(reach=float('inf')), dict(reach=float('nan')), dict(through_walls=2), dict(through_walls=-1),
           dict(positions=odd8), dict(timers=odd4), dict(kinds=odd4), dict(taker=odd4), dict(counts=odd4), dict(agents=None), dict(agents=odd8),
           dict(n_agents=0), dict(n_agents=65), dict(n_envs=0), dict(walls=None), dict(wall_starts=None)]
    for kw in bad:
        assert collect(**kw) == -1, kw
    assert h.ms_host_item_collect(None, 1, 1, p, p, starts.ctypes.data) == -1

    def overlay(n_envs=1, widths=p, **kw):
        spec = dict(n_items=1, n_rays=2, n_origins=1, positions=p, colors=p, origins=p, dirs=p, radius=.1, near_plane=.1, distances=p,
                    indices=None, locations=None, dots=None, screen=None, items=None)
        spec.update(kw)
        return h.ms_host_item_overlay(C.byref(_lib.MsItemOverlay(**spec)), n_envs, widths)

    assert overlay() == 0 and overlay(near_plane=0.) == 0 and overlay(colors=None) == 0
    bad = [dict(n_items=0), dict(n_items=1025), dict(n_rays=0), dict(n_origins=0), dict(n_rays=3, n_origins=2), dict(positions=None),
           dict(origins=None), dict(dirs=None), dict(distances=None), dict(screen=p, colors=None), dict(radius=0.), dict(radius=float('inf')),
           dict(radius=float('nan')), dict(near_plane=-1.), dict(near_plane=float('nan')), dict(positions=odd8), dict(origins=odd8),
           dict(dirs=odd8), dict(colors=odd4), dict(distances=odd4), dict(indices=odd4), dict(locations=odd4), dict(dots=odd4),
           dict(screen=odd4), dict(items=odd4), dict(n_envs=0), dict(indices=p, widths=None)]
    for kw in bad:
        assert overlay(**kw) == -1, kw
    assert overlay(n_envs=2**30, n_rays=4) == -3                         # (N R beyond 2^31 - 1)
    assert h.ms_host_item_overlay(None, 1, p) == -1
    # the launches: a NULL or zeroed scenery, agents and struct
    sc, ag = _lib.MsScenery(), _lib.MsAgents()
    assert h.ms_item_collect(None, None, None, None) == -1 and h.ms_item_overlay(None, None, None) == -1
    assert h.ms_item_collect(C.byref(sc), C.byref(ag), C.byref(_lib.MsItemCollect()), None) == -1
    assert h.ms_item_overlay(C.byref(sc), C.byref(_lib.MsItemOverlay()), None) == -1
    sound = _lib.MsScenery(n_envs=1, n_agents=1, n_model=1, lines_vals=p, lines_widths=p, lines_starts=p, model=p)
    assert h.ms_item_collect(C.byref(sound), None, C.byref(_lib.MsItemCollect()), None) == -1
    assert h.ms_item_collect(C.byref(sound), C.byref(ag), C.byref(_lib.MsItemCollect()), None) == -1
    assert h.ms_item_collect(C.byref(sound), C.byref(_lib.MsAgents(positions=p)), None, None) == -1
    assert h.ms_item_overlay(C.byref(sound), None, None) == -1 and h.ms_item_overlay(C.byref(sound), C.byref(_lib.MsItemOverlay()), None) == -1
    crowd = _lib.MsScenery(n_envs=1, n_agents=65, n_model=1, lines_vals=p, lines_widths=p, lines_starts=p, model=p)
    spec = _lib.MsItemCollect(n_items=1, n_kinds=1, positions=p, timers=p, kinds=p, reach=1., through_walls=1)
    assert h.ms_item_collect(C.byref(crowd), C.byref(_lib.MsAgents(positions=p)), C.byref(spec), None) == -1


# ---------------------------------------------------------------------------------------------------------------------
# the Python layer
# ---------------------------------------------------------------------------------------------------------------------
def test_the_python_calls_refuse_what_they_cannot_do():
    import torch
    from megastep_amd import core, cuda, scene, toys
    scenery = scene.scenery([toys.box()], 2, device='cpu', bake=False)
    cuda.initialize(core.AGENT_RADIUS, 64, 130, 10)
    agents = core._init_agents(1, 2, 'cpu')
    store = cuda.items(1, 5, kinds=[0, 1, 2, 0, 1], colors=(1., .5, 0.), device='cpu')
    assert store.n_kinds == 3 and store.n_items == 5 and store.n_envs == 1 and not store.present().any()
    assert store.positions.shape == (1, 5, 2) and torch.isnan(store.positions).all() and (store.timers == 0).all()
    assert store.kinds.dtype == torch.int32 and store.colors.shape == (1, 5, 3) and store.colors.is_contiguous()
    for bad in (dict(n_items=0), dict(n_items=1025), dict(n_envs=0), dict(kinds=[0, 1]), dict(kinds=[0, 1, 2, 3, 8]), dict(kinds=[-1, 0, 0, 0, 0]),
                dict(kinds=[0., 1., 0., 0., 0.]), dict(n_kinds=9), dict(kinds=[0, 1, 2, 0, 1], n_kinds=2), dict(colors=(1., 1.)),
                dict(colors=torch.ones(4, 3))):
        with pytest.raises(RuntimeError):
            cuda.items(**{**dict(n_envs=1, n_items=5, device='cpu'), **bad})
    with pytest.raises(RuntimeError, match='GPU'):
        cuda.collect_items(scenery, agents, store, .3)
    for bad in (dict(reach=0.), dict(reach=float('inf')), dict(reach='far'), dict(delay=1.5), dict(delay=2**31),
                dict(takers=torch.ones(1, 3, dtype=torch.bool)), dict(takers=torch.ones(1, 2)), dict(reset=torch.ones(2, dtype=torch.bool))):
        with pytest.raises(RuntimeError):
            cuda.collect_items(scenery, agents, store, **{**dict(reach=.3), **bad})
    with pytest.raises(RuntimeError, match='cuda.Items'):
        cuda.collect_items(scenery, agents, store.positions, .3)
    with pytest.raises(RuntimeError, match='agents do not match'):
        cuda.collect_items(scenery, core._init_agents(1, 3, 'cpu'), store, .3)
    with pytest.raises(RuntimeError, match='N = 1'):
        cuda.collect_items(scenery, agents, cuda.items(2, 5, device='cpu'), .3)
    # the overlay: a frame is a Render or a Raycast, with what its rays were
    planes = [torch.zeros((1, 8), dtype=t) for t in (torch.int32, torch.float32, torch.float32, torch.float32)]
    cast = cuda.Raycast(*planes, None)
    origins, dirs = torch.zeros(1, 8, 2), torch.ones(1, 8, 2)
    with pytest.raises(RuntimeError, match='Render or a cuda.Raycast'):
        cuda.overlay_items(store, planes[3], origins=origins, dirs=dirs, scenery=scenery)
    with pytest.raises(RuntimeError, match='origins= and dirs='):
        cuda.overlay_items(store, cast, scenery=scenery)
    with pytest.raises(RuntimeError, match='no distances'):
        cuda.overlay_items(store, cuda.Raycast(planes[0], None, None, None, None), origins=origins, dirs=dirs, scenery=scenery)
    with pytest.raises(RuntimeError, match='R % Q'):
        cuda.overlay_items(store, cast, origins=torch.zeros(1, 3, 2), dirs=dirs, scenery=scenery, near=.1)
    with pytest.raises(RuntimeError, match='scenery='):
        cuda.overlay_items(store, cast, origins=origins, dirs=dirs, near=.1)
    with pytest.raises(RuntimeError, match='radius'):
        cuda.overlay_items(store, cast, origins=origins, dirs=dirs, scenery=scenery, near=.1, radius=0.)
    with pytest.raises(RuntimeError, match='near'):
        cuda.overlay_items(store, cast, origins=origins, dirs=dirs, scenery=scenery, near=-1.)
    with pytest.raises(RuntimeError, match='GPU'):
        cuda.overlay_items(store, cast, origins=origins, dirs=dirs, scenery=scenery, near=.1)
    render = cuda.Render(*[t.view(1, 2, 4) for t in planes], torch.zeros(1, 2, 4, 3))
    with pytest.raises(RuntimeError, match='agents='):
        cuda.overlay_items(store, render, scenery=scenery)
    with pytest.raises(RuntimeError, match='agents do not match'):
        cuda.overlay_items(store, render, agents=core._init_agents(1, 3, 'cpu'), dirs=dirs, scenery=scenery)


def test_the_modules_reward_is_counts_times_values():
    import torch
    from megastep_amd import modules
    counts = torch.tensor([[[2, 0, 1], [0, 0, 0]], [[0, 3, 0], [1, 1, 1]]], dtype=torch.int32)
    reward = modules.Items.reward(counts, torch.tensor([1., -2., .5]))
    assert reward.dtype == torch.float32 and torch.equal(reward, torch.tensor([[2.5, 0.], [-6., -.5]]))
