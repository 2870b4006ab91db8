"""Solid bodies (include/megastep_hip.h, MsBodies) in numpy - body_rule, one binary32 operation a statement, the pair
and wall tests the oracle's own collision_cc and collision_cs with no cull in front - and ms_host_bodies on arrays. A world is
slide_rule's; a store is walker_rule's ``positions`` (N, P, 2), with ``velocities`` where the bodies move."""
import ctypes as C

import numpy as np

from tests.item_rule import F, NAN  # noqa: F401
from tests.slide_rule import STATE, _cc, _cs, _moved, _normalize
from tests.walker_rule import RADIUS, ROOM, random_store  # noqa: F401

KEYS = STATE + ('progress', 'blocker', 'contacts')


def body_rule(w, positions, velocities=None, movement=None, radius=RADIUS, fps=10.):
    """One step of the agents of world ``w`` among the bodies: the state after it, ``progress``, ``blocker`` and ``contacts``."""
    v, spin = _moved(w, movement)
    N, A = spin.shape
    R, fps = F(radius), F(fps)
    out = {k: np.array(w[k], F) for k in STATE}
    out.update(progress=np.ones((N, A), F), blocker=np.full((N, A), -1, np.int32), contacts=np.zeros((N, A), np.int32))
    with np.errstate(all='ignore'):
        u = v/fps
        for n in range(N):
            there = np.flatnonzero(np.isfinite(positions[n]).all(-1))
            moving = velocities is not None
            ub = {k: (F(velocities[n, k]/fps) if moving and np.isfinite(velocities[n, k]).all() else np.zeros(2, F)) for k in there}
            for a in range(A):
                p = w['positions'][n, a]
                xs = [_cc(p, u[n, a], w['positions'][n, b], u[n, b], R) for b in range(A) if b != a] + [_cs(p, u[n, a], row, R) for row in w['walls'][n]]
                cs = {k: _cc(p, u[n, a], positions[n, k], ub[k], R) for k in there}
                x = min([F(1)] + xs + list(cs.values()))
                out['progress'][n, a], out['contacts'][n, a] = x, sum(c < 1 for c in cs.values())
                if x < 1:
                    out['blocker'][n, a] = min([k for k, c in cs.items() if c == x], default=-1)
                    out['velocity'][n, a], out['angvelocity'][n, a] = 0, 0
                else:
                    out['velocity'][n, a], out['angvelocity'][n, a] = v[n, a], spin[n, a]
                out['positions'][n, a] = p + F(x*v[n, a])/fps
                out['angles'][n, a] = _normalize(F(w['angles'][n, a] + F(F(x*spin[n, a])/fps)))
    return out


def host_bodies(w, positions, velocities=None, movement=None, extras=None, radius=RADIUS, fps=10., expect=0, spoil=()):
    """ms_host_bodies over a world, one call. ``extras``: an _lib.MsStepExtras over host arrays the caller keeps alive; ``spoil``:
    (name, value) pairs over the MsBodies' fields and ``n_agents``; ``expect``: the status the call must return."""
    from megastep_amd import _lib
    from tests.item_rule import wall_rows
    N, A = w['angles'].shape
    walls, starts = wall_rows(w['walls'])
    st = {k: np.ascontiguousarray(w[k], F).copy() for k in STATE}
    ag = _lib.MsAgents(st['angles'].ctypes.data, st['positions'].ctypes.data, st['angvelocity'].ctypes.data, st['velocity'].ctypes.data, None, None)
    mv = None
    if movement is not None:
        actions, table = np.ascontiguousarray(movement[0], np.int64), np.ascontiguousarray(movement[1], F)
        mv = C.byref(_lib.MsMovement(actions.ctypes.data, table.ctypes.data, len(table), float(movement[2])))
    positions = np.ascontiguousarray(positions, F)
    velocities = None if velocities is None else np.ascontiguousarray(velocities, F)
    out = dict(st, progress=np.zeros((N, A), F), blocker=np.full((N, A), -7, np.int32), contacts=np.full((N, A), -7, np.int32))
    bd = _lib.MsBodies(positions.shape[1], positions.ctypes.data, None if velocities is None else velocities.ctypes.data,
                       out['blocker'].ctypes.data, out['contacts'].ctypes.data)
    for name, value in spoil:
        if name == 'n_agents':
            A = value
        else:
            setattr(bd, name, value(getattr(bd, name)) if callable(value) else value)
    cfg = _lib.MsConfig(float(radius), 8, 90., float(fps))
    status = _lib.lib().ms_host_bodies(walls.ctypes.data, starts.ctypes.data, N, A, C.byref(ag), mv, None if extras is None else C.byref(extras),
                                       C.byref(bd), out['progress'].ctypes.data, C.byref(cfg))
    assert status == expect, status
    return out
