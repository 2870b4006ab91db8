"""Rollouts among bodies on the CPU: ms_host_rollouts_bodies against H chained ms_host_bodies steps, the store moved on
between them in numpy binary32, as bits in all ten outputs; and the refusals, none of which gets to a launch."""
import ctypes as C

import numpy as np
import pytest

from tests.body_rule import F, NAN, RADIUS, ROOM, host_bodies
from tests.item_rule import same
from tests.rollout_rule import FIELDS, _empty
from tests.slide_rule import STATE, world

KEYS = FIELDS + ('body_stops', 'first_blocker')
blank = lambda N, A, K, H: dict(_empty(N, A, K, H), body_stops=np.zeros((N, A, K), np.int32), first_blocker=np.full((N, A, K), -1, np.int32))
TABLE = F([[0, 0, 0], [2, 0, 0], [0, 2, 0], [-2, 0, 30]])                  # (row 0: all zero - an agent at rest stays at rest on it)
KEEP, FPS, P = .875, 10., 8
PLANS = {1: np.array([[1], [2], [3]]), 6: np.array([[1]*6, [2]*6, [3, 3, 0, 0, 3, 3]])}


def room(A):
    """walker_rule's room, an agent at (1, 2) heading along +x - and, A = 2, one at rest beyond the partition - among six bodies:
    one a step ahead of each agent, one above, two out of the way; slots 2 and 5 absent; slot 4's velocity is not finite."""
    w = world([ROOM], [[(1., 2.), (6.5, 1.)][:A]], velocity=[[(.5, .2), (0., 0.)][:A]], angvelocity=[[10., 0.][:A]])
    positions, velocities = np.full((1, P, 2), NAN, F), np.zeros((1, P, 2), F)
    for k, (p, v) in {0: ((1.5, 2.), (-1., 0.)), 1: ((1., 2.6), (0., .5)), 3: ((6.95, 1.), (0., 0.)), 4: ((6.5, 1.45), (NAN, -3.)),
                      6: ((3., .5), (1., 1.)), 7: ((7.5, 3.5), (0., 0.))}.items():
        positions[0, k], velocities[0, k] = p, v
    return w, positions, velocities


def stepped(w, plans, positions, velocities):
    """The reference: per agent and plan H ms_host_bodies steps of a copy of the env, the others at rest on row 0, the bodies moved on between."""
    A, (K, H) = w['angles'].shape[1], plans.shape
    out = blank(1, A, K, H)
    with np.errstate(invalid='ignore'):
        u = None if velocities is None else np.where(np.isfinite(velocities).all(-1, keepdims=True), velocities/F(FPS), F(0)).astype(F)
    for a in range(A):
        for k in range(K):
            c = dict(w, **{key: w[key].copy() for key in STATE})
            rest = np.arange(A) != a
            c['velocity'][0, rest], c['angvelocity'][0, rest] = 0, 0
            q, books = positions.copy(), out
            for h in range(H):
                actions = np.where(rest, 0, plans[k, h])[None]
                step = host_bodies(c, q, None if u is None else velocities, (actions, TABLE, KEEP), fps=FPS)
                c.update({key: step[key] for key in STATE})
                x, blocker = step['progress'][0, a], step['blocker'][0, a]
                books['trail'][0, a, k, h] = step['positions'][0, a]
                books['progress'][0, a, k] = min(books['progress'][0, a, k], x)
                if x < 1:
                    books['stops'][0, a, k] += 1
                    books['first_stop'][0, a, k] = min(books['first_stop'][0, a, k], h)
                if blocker >= 0:
                    if not books['body_stops'][0, a, k]:
                        books['first_blocker'][0, a, k] = blocker
                    books['body_stops'][0, a, k] += 1
                if u is not None:
                    q = q + u
            for key in STATE:
                out[key][0, a, k] = c[key][0, a]
    return out


def host_rollouts_bodies(w, plans, table, keep, others, positions, velocities, radius=RADIUS, fps=FPS, mask=None, spoil=None, expect=0):
    """ms_host_rollouts_bodies, env by env: the ten outputs. ``spoil``: (field, change) or ('bodies', None); ``expect``: every call's status."""
    from megastep_amd import _lib
    plans, table = np.ascontiguousarray(plans, np.int64), np.ascontiguousarray(table, F)
    N, A = w['angles'].shape
    K, H = plans.shape[-2:]
    out = blank(N, A, K, H)
    cfg = _lib.MsConfig(float(radius), 8, 90., float(fps))
    for n in range(N):
        walls = np.ascontiguousarray(w['walls'][n], F).reshape(-1, 4)
        st = {k: np.ascontiguousarray(w[k][n], F) for k in ('angles', 'positions', 'angvelocity', 'velocity')}
        ag = _lib.MsAgents(st['angles'].ctypes.data, st['positions'].ctypes.data, st['angvelocity'].ctypes.data, st['velocity'].ctypes.data, None, None)
        acts = plans if plans.ndim == 2 else np.ascontiguousarray(plans[n])
        m = None if mask is None else np.ascontiguousarray(mask[n], np.uint8)
        env = {k: np.ascontiguousarray(out[k][n]) for k in KEYS}
        q = np.ascontiguousarray(positions[n], F)
        v = None if velocities is None else np.ascontiguousarray(velocities[n], F)
        r = _lib.MsRollouts(K, H, acts.ctypes.data, int(plans.ndim == 2), table.ctypes.data, len(table), float(keep), int(others == 'rest'),
                            None if m is None else m.ctypes.data, *(env[k].ctypes.data for k in FIELDS))
        rb = _lib.MsRolloutBodies(q.shape[0], q.ctypes.data, None if v is None else v.ctypes.data, env['body_stops'].ctypes.data,
                                  env['first_blocker'].ctypes.data)
        if spoil and spoil[1]:
            s = rb if hasattr(rb, spoil[0]) else r                          # (`positions`: the store's)
            setattr(s, spoil[0], spoil[1](getattr(s, spoil[0])))
        status = _lib.lib().ms_host_rollouts_bodies(walls.ctypes.data if len(walls) else None, len(walls), C.byref(ag), A, C.byref(r),
                                                    None if spoil == ('bodies', None) else C.byref(rb), C.byref(cfg))
        assert status == expect, status
        for k in KEYS:
            out[k][n] = env[k]
    return out


@pytest.mark.parametrize('moving', [False, True], ids=['rest', 'moving'])
@pytest.mark.parametrize('H', [1, 6])
@pytest.mark.parametrize('A', [1, 2])
def test_the_host_statement_is_the_step_among_bodies_chained(oracle, A, H, moving):
    w, positions, velocities = room(A)
    velocities = velocities if moving else None
    want = stepped(w, PLANS[H], positions, velocities)
    body, free = (want['body_stops'] > 0).mean(), (want['body_stops'] == 0).mean()      # (of the reference alone)
    assert body >= .25 and free >= .25, (body, free)
    same(host_rollouts_bodies(w, PLANS[H], TABLE, KEEP, 'rest' if A > 1 else None, positions, velocities), want, KEYS)


SPOILS = {'no store': ('bodies', None), 'no positions': ('positions', lambda p: 0), 'positions off 8': ('positions', lambda p: p + 4),
          'velocities off 8': ('velocities', lambda p: p + 4), 'body_stops off 4': ('body_stops', lambda p: p + 2),
          'first_blocker off 4': ('first_blocker', lambda p: p + 2), 'no slot': ('n_slots', lambda n: 0), '1025 slots': ('n_slots', lambda n: 1025),
          'slide': ('slide', lambda s: 1)}


@pytest.mark.parametrize('what', SPOILS)
def test_arguments_are_refused(oracle, what):
    w, positions, velocities = room(2)
    host_rollouts_bodies(w, PLANS[6], TABLE, KEEP, 'rest', positions, velocities, spoil=SPOILS[what], expect=-1)


def test_a_pinned_scheme_and_null_arguments_are_refused(oracle):
    from megastep_amd import _lib
    w, positions, velocities = room(1)
    h = _lib.lib()
    try:
        assert h.ms_debug_rollout_scheme(1) == 0
        host_rollouts_bodies(w, PLANS[1], TABLE, KEEP, None, positions, velocities, expect=-1)
        assert h.ms_debug_rollout_scheme(0) == 0
        host_rollouts_bodies(w, PLANS[1], TABLE, KEEP, None, positions, velocities)
    finally:
        h.ms_debug_rollout_scheme(-1)
    cfg = _lib.MsConfig(RADIUS, 8, 90., FPS)
    for args in ([None]*4, [C.byref(s()) for s in (_lib.MsScenery, _lib.MsAgents, _lib.MsRollouts, _lib.MsRolloutBodies)]):
        assert h.ms_rollouts_bodies(*args, C.byref(cfg), None) == -1         # (the device entry, NULL and zeroed: no launch)
