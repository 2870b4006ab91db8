"""Projectiles (include/megastep_hip.h, MsProjectiles) restated in numpy - fly_rule, one binary32 operation a
statement, a loop per projectile, the fold tests/item_rule.py's - and ms_host_projectiles on numpy arrays."""
import ctypes

import numpy as np

from tests import item_rule as ir
from tests.item_rule import F, NAN, same, wall_rows  # noqa: F401

STORE = ('positions', 'velocities', 'owners', 'timers', 'bounces')
KEYS = STORE + ('struck', 'ended', 'hits', 'scored', 'misfires')
ROOM = np.array([(0, 0, 8, 0), (8, 0, 8, 4), (8, 4, 0, 4), (0, 4, 0, 0), (4, 1, 6, 3)], F)     # the 8 x 4 box and a diagonal partition


def model():
    from megastep_amd import scene
    return np.ascontiguousarray(scene.agent_model(), F).reshape(-1, 4)


def store(N, A, S, shots=()):
    """An empty store with `shots` put in: (n, k, p, v, timer, bounces) each."""
    s = dict(positions=np.full((N, A*S, 2), NAN, F), velocities=np.zeros((N, A*S, 2), F), owners=np.tile((np.arange(A*S)//S).astype(np.int32), (N, 1)),
             timers=np.zeros((N, A*S), np.int32), bounces=np.zeros((N, A*S), np.int32))
    for n, k, p, v, timer, bounces in shots:
        s['positions'][n, k], s['velocities'][n, k], s['timers'][n, k], s['bounces'][n, k] = p, v, timer, bounces
    return s


def random_store(N, A, S, lo, hi, seed, speed=8.):
    """Two thirds of the slots in flight between lo[n] and hi[n], every direction, a third of them slow, timers 1..8, bounces 0..3."""
    rng = np.random.RandomState(seed)
    s, P = store(N, A, S), A*S
    heading = rng.uniform(0, 2*np.pi, (N, P))
    s['positions'][:] = np.stack([rng.uniform(lo[n], hi[n], (P, 2)) for n in range(N)])
    s['velocities'][:] = np.stack([np.cos(heading), np.sin(heading)], -1)*(speed*rng.choice([.05, .6, 1.], (N, P, 1)))
    s['positions'][rng.rand(N, P) < .34] = NAN
    s['timers'][:], s['bounces'][:] = rng.randint(1, 9, (N, P)), rng.randint(0, 4, (N, P))
    return s


def bodies(mdl, agents, angles):
    """The A M rows of one env's agents at their poses (draw_kernel, kernels.cu:305-314), and the headings (s, c)."""
    from oracle import oracle as O
    rows, poses = [], []
    for (px, py), angle in zip(agents, angles):
        s, c = (F(v) for v in O.sincospi(F(F(angle)/F(180))))
        poses.append((s, c))
        rows += [(F(F(c*ax) - F(s*ay)) + px, F(F(s*ax) + F(c*ay)) + py, F(F(c*bx) - F(s*by)) + px, F(F(s*bx) + F(c*by)) + py) for ax, ay, bx, by in mdl]
    return np.array(rows, F).reshape(-1, 4), poses


def fly_rule(walls, mdl, agents, angles, store, fire=None, reset=None, speed=8., muzzle=.25, life=64, bounces=0, restitution=1., fps=10.,
             legs=None):
    """One tick: the store after it and the records. `legs`: a list that takes (x0, y0, x1, y1) of every leg flown through the air."""
    agents, angles = np.asarray(agents, F), np.asarray(angles, F)
    (N, A), M = angles.shape, len(mdl)
    out = {k: np.array(store[k]) for k in STORE}
    P, S = out['positions'].shape[1], out['positions'].shape[1]//A
    out.update(struck=np.full((N, P), -1, np.int32), ended=np.full((N, P), 4, np.uint8), hits=np.zeros((N, A), np.int32),
               scored=np.zeros((N, A), np.int32), misfires=np.zeros((N, A), np.uint8))
    for n in range(N):
        pos, vel = out['positions'][n], out['velocities'][n]
        if reset is not None and reset[n]:
            pos[:], out['timers'][n], out['bounces'][n] = NAN, 0, 0
            continue
        with np.errstate(all='ignore'):
            body, poses = bodies(mdl, agents[n], angles[n])
        for a in range(A):
            if fire is None or not fire[n, a] or not (np.isfinite(agents[n, a]).all() and np.isfinite(angles[n, a])):
                continue
            free = [k for k in range(a*S, a*S + S) if not np.isfinite(pos[k]).all()]
            if not free:
                out['misfires'][n, a] = 1
                continue
            (s, c), k = poses[a], free[0]
            pos[k] = agents[n, a, 0] + F(F(muzzle)*c), agents[n, a, 1] + F(F(muzzle)*s)
            vel[k] = F(F(speed)*c), F(F(speed)*s)
            out['owners'][n, k], out['timers'][n, k], out['bounces'][n, k] = a, life, bounces
        rows = np.asarray(walls[n], F).reshape(-1, 4)
        for k in range(P):
            if np.isfinite(pos[k]).all():
                with np.errstate(all='ignore'):
                    _flight(n, k, out, body, rows, A*M, M, F(restitution), F(fps), [] if legs is None else legs)
                if out['struck'][n, k] >= 0:
                    out['hits'][n, out['struck'][n, k]] += 1
                    if 0 <= out['owners'][n, k] < A:
                        out['scored'][n, out['owners'][n, k]] += 1
    return out


def _flight(n, k, out, body, rows, AF, M, rest, fps, legs):
    one = F(1)
    (px, py), (vx, vy) = out['positions'][n, k], out['velocities'][n, k]
    owner, left, prev, ended = out['owners'][n, k], one, -1, 0
    r = F(F(abs(vx/fps) + abs(vy/fps))*F(1.01)) + F(1e-3)
    bx0, by0, bx1, by1 = px - r, py - r, px + r, py + r
    meets = ~np.isnan(rows).any(1) & (np.minimum(rows[:, 0], rows[:, 2]) <= bx1) & (np.maximum(rows[:, 0], rows[:, 2]) >= bx0) & \
        (np.minimum(rows[:, 1], rows[:, 3]) <= by1) & (np.maximum(rows[:, 1], rows[:, 3]) >= by0)
    for _ in range(4):
        rux, ruy = F(vx/fps)*left, F(vy/fps)*left
        rlen = np.sqrt(F(rux*rux) + F(ruy*ruy))
        if not rlen > 0:
            break
        f = dict(s=np.array([1.001], F), idx=np.array([-1], np.int32), t=np.array([NAN], F), vx=np.zeros(1, F), vy=np.zeros(1, F))
        at = [np.array([v], F) for v in (px, py, rux, ruy)]
        for i in range(AF):
            if i//M != owner:
                ir.fold(*at, F(0), body[i], i, f)
        for l in np.flatnonzero(meets):
            if AF + l != prev:
                ir.fold(*at, F(0), rows[l], AF + l, f)
        idx, s = int(f['idx'][0]), f['s'][0]
        if idx < 0 or (idx >= AF and out['bounces'][n, k] > 0):
            go = one if idx < 0 else max(min(s, one) - F(1e-3)/rlen, F(0))
            qx, qy = px + F(rux*go), py + F(ruy*go)
            legs.append((px, py, qx, qy))
            px, py = qx, qy
        if idx >= 0 and idx < AF:
            out['struck'][n, k] = idx//M
        if idx < AF or out['bounces'][n, k] == 0:
            ended = 0 if idx < 0 else 1 if idx < AF else 2
            break
        out['bounces'][n, k] -= 1
        left = left*(one - min(s, one))
        nx, ny = -f['vy'][0], f['vx'][0]
        kk = F((one + rest)*F(F(vx*nx) + F(vy*ny)))/F(F(nx*nx) + F(ny*ny))
        vx, vy = vx - F(kk*nx), vy - F(kk*ny)
        prev = idx
    if ended == 0:
        out['timers'][n, k] -= 1
        ended = 3 if out['timers'][n, k] == 0 else 0
    out['positions'][n, k], out['velocities'][n, k], out['ended'][n, k] = (NAN, NAN) if ended else (px, py), (vx, vy), ended


def host_fly(walls, mdl, agents, angles, store, fire=None, reset=None, speed=8., muzzle=.25, life=64, bounces=0, restitution=1., fps=10.,
             expect=0, spoil=()):
    """ms_host_projectiles on numpy arrays. `spoil`: (name, value) pairs over the struct's fields and the other arguments."""
    from megastep_amd import _lib
    agents, angles, mdl = np.ascontiguousarray(agents, F), np.ascontiguousarray(angles, F), np.ascontiguousarray(mdl, F)
    out = {k: np.ascontiguousarray(store[k]).copy() for k in STORE}
    (N, A), P = angles.shape, out['positions'].shape[1]
    out.update(struck=np.full((N, P), -7, np.int32), ended=np.full((N, P), 9, np.uint8), hits=np.full((N, A), -7, np.int32),
               scored=np.full((N, A), -7, np.int32), misfires=np.full((N, A), 9, np.uint8))
    flags = [None if a is None else np.ascontiguousarray(a, np.uint8) for a in (fire, reset)]
    rows, starts = wall_rows(walls)
    ptr = lambda a: None if a is None else a.ctypes.data
    spec = _lib.MsProjectiles(P, P//A, *(out[k].ctypes.data for k in STORE), ptr(flags[0]), ptr(flags[1]), float(speed), float(muzzle), int(life),
                              int(bounces), float(restitution), float(fps), *(out[k].ctypes.data for k in KEYS[5:]))
    args = dict(n_envs=N, n_agents=A, agents=agents.ctypes.data, angles=angles.ctypes.data, model=mdl.ctypes.data, n_model=len(mdl),
                walls=rows.ctypes.data, starts=starts.ctypes.data)
    for name, value in spoil:
        now = args[name] if name in args else getattr(spec, name)
        value = value(now) if callable(value) else value
        args.__setitem__(name, value) if name in args else setattr(spec, name, value)
    assert _lib.lib().ms_host_projectiles(ctypes.byref(spec), *args.values()) == expect
    return out
