"""Solid bodies on the CPU: the serial host statement of the kernel's own per-pair functions (ms_host_bodies) against
the numpy rule over the oracle's collision tests (tests/body_rule.py), as bits in every output, in walker_rule's box room with its
diagonal partition; an empty store against the plain step; and the refusals."""
import ctypes as C

import numpy as np
import pytest

from tests.body_rule import F, KEYS, NAN, RADIUS, ROOM, body_rule, host_bodies, random_store
from tests.item_rule import same
from tests.slide_rule import STATE, plain_rule, world

P = 8
FAR = ((7., .5), (0., 0.))                                                  # an agent that stands in a corner, out of everybody's way
# a case an env: two agents (position, velocity m/s) and the bodies {slot: (position, velocity)} - the slots between them absent
CASES = dict(
    straight_at_one=([((1., 2.), (3., 0.)), FAR], {3: ((1.5, 2.), (0., 0.))}),
    two_at_equal_distance=([((1., 2.), (3., 0.)), FAR], {5: ((1.5, 2.125), (0., 0.)), 2: ((1.5, 1.875), (0., 0.))}),
    a_wall_is_nearer=([((7.5, 2.), (5., 0.)), FAR], {4: ((8.2, 2.), (0., 0.))}),
    one_for_two_agents=([((2., 1.), (3., 0.)), ((3., 1.), (-3., 0.))], {0: ((2.5, 1.), (0., 0.))}),
    head_on_and_running_away=([((1., 3.), (3., 0.)), ((5., 3.5), (3., 0.))], {1: ((1.5, 3.), (-3., 0.)), 7: ((5.5, 3.5), (2.9, 0.))}),
    a_nan_velocity=([((1., 1.), (0., 3.)), FAR], {6: ((1., 1.5), (NAN, -9.))}),
    a_nan_pose=([((NAN, 2.), (3., 0.)), ((2., 3.), (0., -3.))], {2: ((2., 2.5), (0., 0.)), 3: ((1., 2.), (0., 0.))}))


def cases():
    N = len(CASES)
    w = world([ROOM]*N, [[a[0] for a in agents] for agents, _ in CASES.values()], velocity=[[a[1] for a in agents] for agents, _ in CASES.values()])
    positions, velocities = np.full((N, P, 2), NAN, F), np.zeros((N, P, 2), F)
    for n, (_, bodies) in enumerate(CASES.values()):
        for k, (p, v) in bodies.items():
            positions[n, k], velocities[n, k] = p, v
    return w, positions, velocities


@pytest.mark.parametrize('moving', [False, True], ids=['rest', 'moving'])
def test_the_host_statement_is_the_rule_case_by_case(oracle, moving):
    w, positions, velocities = cases()
    want = body_rule(w, positions, velocities if moving else None)
    same(host_bodies(w, positions, velocities if moving else None), want, KEYS)
    n = {name: i for i, name in enumerate(CASES)}
    x, blocker, contacts = want['progress'], want['blocker'], want['contacts']
    assert x[n['straight_at_one'], 0] < 1 and blocker[n['straight_at_one']].tolist() == [3, -1]
    assert blocker[n['two_at_equal_distance'], 0] == 2 and contacts[n['two_at_equal_distance'], 0] == 2
    assert x[n['a_wall_is_nearer'], 0] < 1 and blocker[n['a_wall_is_nearer'], 0] == -1 and contacts[n['a_wall_is_nearer'], 0] == 1
    assert blocker[n['one_for_two_agents']].tolist() == [0, 0]
    # head-on the body takes half the gap; the one running away at nearly the agent's speed is only met where it stands still
    e = n['head_on_and_running_away']
    assert blocker[e].tolist() == ([1, -1] if moving else [1, 7]) and (x[e, 0] < .5) == moving
    assert blocker[n['a_nan_velocity'], 0] == 6                             # (at rest either way)
    assert x[n['a_nan_pose'], 0] == 1 and contacts[n['a_nan_pose']].tolist() == [0, 1]


@pytest.mark.parametrize('A,slots,moving', [(1, 5, False), (3, 20, True), (4, 70, False)])
def test_the_host_statement_is_the_rule_in_a_crowded_room(oracle, A, slots, moving):
    """Random bodies in the room, half of them clustered, a third of the slots absent; the agents start a step from one and head
    its way, one action each from a table - the movement rides in the call."""
    rng = np.random.RandomState(slots)
    store, _ = random_store(2, slots, [(0, 0)]*2, [(8, 4)]*2, seed=slots)
    spots = np.stack([store['positions'][n][np.isfinite(store['positions'][n, :, 0])][np.arange(A) % 3] for n in range(2)])
    w = world([ROOM]*2, spots + rng.uniform(.3, .5, (2, A, 1))*F([1, .3]), velocity=rng.uniform(-3, -1, (2, A, 2)), angvelocity=rng.uniform(-90, 90, (2, A)))
    movement = (rng.randint(0, 3, (2, A)), F([[0, 0, 0], [0, 2, 0], [-2, 0, 30]]), .875)
    velocities = store['velocities'] if moving else None
    want = body_rule(w, store['positions'], velocities, movement)
    same(host_bodies(w, store['positions'], velocities, movement), want, KEYS)
    assert (want['contacts'] > 0).any()


def test_an_empty_store_is_the_plain_step(oracle):
    rng = np.random.RandomState(3)
    w = world([ROOM]*3, rng.uniform((.3, .3), (7.7, 3.7), (3, 4, 2)), velocity=rng.uniform(-4, 4, (3, 4, 2)), angvelocity=rng.uniform(-90, 90, (3, 4)))
    w['positions'][0, 1] = w['positions'][0, 0] + F([.25, .05])            # (a pair a step apart)
    got = host_bodies(w, np.full((3, P, 2), NAN, F), np.zeros((3, P, 2), F))
    plain = plain_rule(w, RADIUS, 10.)
    same(got, plain, STATE + ('progress',))
    assert (got['progress'] < 1).any() and (got['blocker'] == -1).all() and (got['contacts'] == 0).all()


@pytest.mark.parametrize('spoil', [('positions', None), ('positions', lambda p: p + 4), ('velocities', lambda p: p + 4), ('blocker', lambda p: p + 2),
                                   ('contacts', lambda p: p + 2), ('n_slots', 0), ('n_slots', 1025), ('n_agents', 65)],
                         ids=['no positions', 'positions off 8', 'velocities off 8', 'blocker off 4', 'contacts off 4', 'no slot', '1025 slots', '65 agents'])
def test_arguments_are_refused(oracle, spoil):
    w, positions, velocities = cases()
    host_bodies(w, positions, velocities, spoil=[spoil], expect=-1)


def test_a_null_store_is_refused(oracle):
    from megastep_amd import _lib
    w, positions, _ = cases()
    h, cfg, p = _lib.lib(), _lib.MsConfig(RADIUS, 8, 90., 10.), positions.ctypes.data
    ag = _lib.MsAgents(p, p, p, p, None, None)
    assert h.ms_host_bodies(p, p, 1, 1, C.byref(ag), None, None, None, p, C.byref(cfg)) == -1
    assert h.ms_bodies_physics(None, None, None, None, None, None, C.byref(cfg), None) == -1
