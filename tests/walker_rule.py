"""Walkers (include/megastep_hip.h, MsWalkers) in numpy - walk_rule, one binary32 operation a statement, a loop per
walker, the pair and wall tests the oracle's own collision_cc and collision_cs with no cull in front - and ms_host_walkers on arrays."""
import ctypes

import numpy as np

from tests.item_rule import F, NAN, same, wall_rows  # noqa: F401

STORE = ('positions', 'velocities')
KEYS = STORE + ('progress', 'blocked', 'bumps', 'close')
ROOM = np.array([(0, 0, 8, 0), (8, 0, 8, 4), (8, 4, 0, 4), (0, 4, 0, 0), (4, 1, 6, 3)], F)     # the 8 x 4 box and a diagonal partition
RADIUS = .15


def store(N, P, walkers=(), speed=1.):
    """An empty store with `walkers` put in: (n, k, p, v) each; and its speeds."""
    s = dict(positions=np.full((N, P, 2), NAN, F), velocities=np.zeros((N, P, 2), F), speeds=np.full((N, P), speed, F))
    for n, k, p, v in walkers:
        s['positions'][n, k], s['velocities'][n, k] = p, v
    return s


def random_store(N, P, lo, hi, seed, fast=None):
    """Two thirds of the slots present between lo[n] and hi[n], half of them in a cluster so that bodies meet, speeds .4 to 1.6, velocities
    up to 1 m/s; targets a few metres off, every ninth a NaN. `fast`: {slot: speed} - present in every env, their target five metres away."""
    rng = np.random.RandomState(seed)
    s, fast = store(N, P), {k: v for k, v in (fast or {}).items() if k < P}
    for n in range(N):
        spread = rng.uniform(lo[n], hi[n], (P, 2))
        heart = rng.uniform(lo[n], hi[n], 2) + rng.uniform(-1, 1, (P, 2))*min(.2*np.sqrt(P), 3.)
        s['positions'][n] = np.where(rng.rand(P, 1) < .5, spread, heart)
    s['velocities'][:] = rng.uniform(-1, 1, (N, P, 2))
    s['speeds'][:] = rng.uniform(.4, 1.6, (N, P))
    absent = rng.rand(N, P) < .34
    absent[:, list(fast)] = False
    s['positions'][absent] = NAN
    towards = (s['positions'] + rng.uniform(-3, 3, (N, P, 2))).astype(F)
    towards[:, ::9] = NAN
    for k, speed in fast.items():
        s['speeds'][:, k], towards[:, k] = speed, s['positions'][:, k] + np.array([4, 3], F)
    return s, towards


def _oracle():
    from oracle import oracle as O
    return O.lib()


_cc = lambda p, u, o, ou, radius: F(_oracle().oracle_collision_cc(*p, *u, *o, *ou, radius))
_cs = lambda p, u, row, radius: F(_oracle().oracle_collision_cs(*p, *u, *row, radius))


def walk_rule(walls, agents, store, towards, personal=.6, push=1., keep=.5, agents_push=True, reset=None, fps=10., radius=RADIUS, steps=None):
    """One tick: the store after it and the records. `steps`: a list that takes (x0, y0, x1, y1) of every walker's move."""
    agents, towards = np.asarray(agents, F), np.asarray(towards, F)
    (N, A), P = agents.shape[:2], store['positions'].shape[1]
    personal, push, keep, fps, radius, one, zero = F(personal), F(push), F(keep), F(fps), F(radius), F(1), np.zeros(2, F)
    out = {k: np.array(store[k]) for k in STORE}
    out.update(progress=np.full((N, P), NAN, F), blocked=np.full((N, P), 4, np.uint8), bumps=np.zeros((N, A), np.int32), close=np.zeros((N, A), np.int32))
    with np.errstate(all='ignore'):
        for n in range(N):
            if reset is not None and reset[n]:
                out['positions'][n] = NAN
                continue
            pos, vel = np.array(store['positions'][n], F), np.array(store['velocities'][n], F)           # the start of the tick
            there = np.isfinite(pos).all(-1)
            bodies = [(1, agents[n, a], a) for a in range(A) if np.isfinite(agents[n, a]).all()] + [(2, pos[j], j) for j in range(P) if there[j]]
            v = np.zeros((P, 2), F)
            for k in np.flatnonzero(there):
                p, speed = pos[k], store['speeds'][n, k]
                d = towards[n, k] - p
                l = np.sqrt(F(d[0]*d[0]) + F(d[1]*d[1]))
                pref = zero
                if l > 0:
                    s = F(l*fps)
                    pref = d*F((s if s < speed else speed)/l)
                sep = zero
                for cls, o, j in bodies:
                    if cls == 2 and j == k:
                        continue
                    r = p - o
                    l2 = F(r[0]*r[0]) + F(r[1]*r[1])
                    if 0 < l2 < F(personal*personal):
                        if cls == 1:
                            out['close'][n, j] += 1
                        if cls == 2 or agents_push:
                            lj = np.sqrt(l2)
                            sep = sep + r*F(F(push*F(personal - lj))/F(personal*lj))
                want = pref + sep
                wl = np.sqrt(F(want[0]*want[0]) + F(want[1]*want[1]))
                if wl > speed:
                    want = want*F(speed/wl)
                vk = keep*vel[k] + F(one - keep)*want
                v[k] = vk if np.isfinite(vk).all() else zero
            u = v/fps
            rows = np.asarray(walls[n], F).reshape(-1, 4)
            for k in np.flatnonzero(there):
                best = (one, 0)
                for cls, o, j in bodies:
                    if cls == 2 and j == k:
                        continue
                    c = _cc(pos[k], u[k], o, u[j] if cls == 2 else zero, radius)
                    if cls == 1 and c < 1:
                        out['bumps'][n, j] += 1
                    best = min(best, (c, cls)) if c < 1 else best
                for row in rows:
                    c = _cs(pos[k], u[k], row, radius)
                    best = min(best, (c, 3)) if c < 1 else best
                x = best[0]
                new = pos[k] + F(x*v[k])/fps
                if steps is not None:
                    steps.append((*pos[k], *new))
                out['positions'][n, k], out['velocities'][n, k] = new, (zero if x < 1 else v[k])
                out['progress'][n, k], out['blocked'][n, k] = x, best[1]
    return out


def host_walk(walls, agents, store, towards, personal=.6, push=1., keep=.5, agents_push=True, reset=None, fps=10., radius=RADIUS,
              expect=0, spoil=()):
    """ms_host_walkers on numpy arrays. `spoil`: (name, value) pairs over the struct's fields and the other arguments."""
    from megastep_amd import _lib
    agents, towards, speeds = (np.ascontiguousarray(a, F) for a in (agents, towards, store['speeds']))
    out = {k: np.ascontiguousarray(store[k]).copy() for k in STORE}
    (N, A), P = agents.shape[:2], out['positions'].shape[1]
    out.update(progress=np.full((N, P), 7, F), blocked=np.full((N, P), 9, np.uint8), bumps=np.full((N, A), -7, np.int32), close=np.full((N, A), -7, np.int32))
    reset = None if reset is None else np.ascontiguousarray(reset, np.uint8)
    rows, starts = wall_rows(walls)
    spec = _lib.MsWalkers(P, out['positions'].ctypes.data, out['velocities'].ctypes.data, speeds.ctypes.data, towards.ctypes.data,
                          None if reset is None else reset.ctypes.data, float(personal), float(push), float(keep), int(agents_push), float(fps),
                          float(radius), *(out[k].ctypes.data for k in KEYS[2:]))
    args = dict(n_envs=N, n_agents=A, agents=agents.ctypes.data, walls=rows.ctypes.data, starts=starts.ctypes.data)
    for name, value in spoil:
        now = args[name] if name in args else getattr(spec, name)
        value = value(now) if callable(value) else value
        args.__setitem__(name, value) if name in args else setattr(spec, name, value)
    assert _lib.lib().ms_host_walkers(ctypes.byref(spec), *args.values()) == expect
    return out
