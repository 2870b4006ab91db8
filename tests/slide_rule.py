"""The sliding step's rule (MsSlide) restated in numpy - scalar float32 operations in the order the rule is written,
around the CPU oracle's collision_cs and collision_cc, the movement step through ms_host_move_velocity - and the host statement
ms_host_slide driven over whole worlds: what tests/test_slide_host.py holds against each other and tests/test_gpu_slide.py holds
the kernel to. A world is rollout_rule's: ``walls`` (one (W, 4) float32 array per env: the static rows) and the agents'
``positions`` (N, A, 2), ``angles`` (N, A), ``velocity`` (N, A, 2), ``angvelocity`` (N, A)."""
import ctypes as C
import numpy as np
from oracle import oracle as O
from tests.rollout_rule import host_move_velocity

FIELDS = ('positions', 'angles', 'velocity', 'angvelocity', 'progress', 'slid', 'stopped')
STATE = ('positions', 'angles', 'velocity', 'angvelocity')
_f = np.float32


def world(walls, positions, angles=None, velocity=None, angvelocity=None):
    """A world from lists: ``walls`` one array of rows per env, ``positions`` (N, A, 2)."""
    positions = np.asarray(positions, _f)
    N, A = positions.shape[:2]
    z = lambda x, shape: np.zeros(shape, _f) if x is None else np.asarray(x, _f).reshape(shape).copy()
    return dict(walls=[np.asarray(w, _f).reshape(-1, 4) for w in walls], positions=positions.copy(), angles=z(angles, (N, A)),
                velocity=z(velocity, (N, A, 2)), angvelocity=z(angvelocity, (N, A)))


def copy(w):
    return dict(walls=[x.copy() for x in w['walls']], **{k: w[k].copy() for k in STATE})


def _cs(p, u, row, R):
    return _f(O.lib().oracle_collision_cs(p[0], p[1], u[0], u[1], row[0], row[1], row[2], row[3], R))


def _cc(p, u, pb, ub, R):
    return _f(O.lib().oracle_collision_cc(p[0], p[1], u[0], u[1], pb[0], pb[1], ub[0], ub[1], R))


def _normalize(a):
    return _f(O.lib().oracle_normalize_degrees(_f(a)))


def _unit(d):
    l = _f(np.sqrt(_f(_f(d[0]*d[0]) + _f(d[1]*d[1]))))
    if not (l > 0) or not np.isfinite(l):
        return None
    return (_f(_f(d[0]/l) + _f(0)), _f(_f(d[1]/l) + _f(0)))


def _normal_wall(p1, row):
    a, ab = (row[0], row[1]), (_f(row[2] - row[0]), _f(row[3] - row[1]))
    pa = (_f(p1[0] - a[0]), _f(p1[1] - a[1]))
    t = _f(_f(_f(pa[0]*ab[0]) + _f(pa[1]*ab[1]))/_f(_f(ab[0]*ab[0]) + _f(ab[1]*ab[1])))
    t = _f(0) if np.isnan(t) else min(max(t, _f(0)), _f(1))
    q = (_f(a[0] + _f(t*ab[0])), _f(a[1] + _f(t*ab[1])))
    return _unit((_f(p1[0] - q[0]), _f(p1[1] - q[1])))


def _normal_agent(p1, pb, ub, x1):
    q = (_f(pb[0] + _f(x1*ub[0])), _f(pb[1] + _f(x1*ub[1])))
    return _unit((_f(p1[0] - q[0]), _f(p1[1] - q[1])))


def _less(k, best):
    """The lexicographic order of (vn, n.x, n.y) under float <."""
    if best is None:
        return True
    for a, b in zip(k, best):
        if a < b:
            return True
        if b < a:
            return False
    return False


def step_env(walls, p, ang, v, w, R, fps, bounce, slide=True):
    """One env, one step, the movement already made: the rule on (A, 2) / (A,) float32 arrays. Returns the seven outputs;
    ``slide=False``: the plain step by the same statements (every blocked agent a dead stop)."""
    with np.errstate(all='ignore'):
        return _step_env(walls, p, ang, v, w, _f(R), _f(fps), _f(bounce), slide)


def _step_env(walls, p, ang, v, w, R, fps, bounce, slide):
    A = len(ang)
    u = [(_f(v[a][0]/fps), _f(v[a][1]/fps)) for a in range(A)]
    x1 = np.ones(A, _f)
    for a in range(A):
        xs = [_cc(p[a], u[a], p[b], u[b], R) for b in range(A) if b != a] + [_cs(p[a], u[a], row, R) for row in walls]
        x1[a] = min([_f(1)] + xs)
    p1, ang1, v2, u2, r1, slides = [], [], [], [], [], []
    for a in range(A):
        x = x1[a]
        p1.append((_f(p[a][0] + _f(_f(x*v[a][0])/fps)), _f(p[a][1] + _f(_f(x*v[a][1])/fps))))
        ang1.append(_normalize(_f(ang[a] + _f(_f(x*w[a])/fps))))
        best = None
        if slide and x < 1:
            normals = [_normal_agent(p1[a], p[b], u[b], x) for b in range(A) if b != a and _cc(p[a], u[a], p[b], u[b], R) == x]
            normals += [_normal_wall(p1[a], row) for row in walls if _cs(p[a], u[a], row, R) == x]
            for n in normals:
                if n is not None:
                    k = (_f(_f(v[a][0]*n[0]) + _f(v[a][1]*n[1])), n[0], n[1])
                    if _less(k, best):
                        best = k
        if best is not None and best[0] < 0:
            k = _f(_f(_f(1) + bounce)*best[0])
            vv = (_f(v[a][0] - _f(k*best[1])), _f(v[a][1] - _f(k*best[2])))
            r = _f(_f(1) - x)
            slides.append(True); v2.append(vv); r1.append(r)
            u2.append((_f(_f(vv[0]*r)/fps), _f(_f(vv[1]*r)/fps)))
        else:
            slides.append(False); v2.append((v[a][0], v[a][1])); r1.append(_f(0)); u2.append((_f(0), _f(0)))
    out = dict(positions=np.zeros((A, 2), _f), angles=np.zeros(A, _f), velocity=np.zeros((A, 2), _f), angvelocity=np.zeros(A, _f),
               progress=x1, slid=np.zeros(A, _f), stopped=np.zeros(A, np.uint8))
    for a in range(A):
        pos, angle, vel, spin, slid, stopped = p1[a], ang1[a], (v[a][0], v[a][1]), w[a], _f(0), False
        if x1[a] < 1 and not slides[a]:
            vel, spin, stopped = (_f(0), _f(0)), _f(0), True
        elif slides[a]:
            xs = [_cc(p1[a], u2[a], p1[b], u2[b], R) for b in range(A) if b != a] + [_cs(p1[a], u2[a], row, R) for row in walls]
            x2 = min([_f(1)] + xs)
            pos = (_f(p1[a][0] + _f(x2*u2[a][0])), _f(p1[a][1] + _f(x2*u2[a][1])))
            angle = _normalize(_f(ang1[a] + _f(_f(x2*_f(r1[a]*w[a]))/fps)))
            slid = _f(x2*r1[a])
            if x2 < 1:
                vel, spin, stopped = (_f(0), _f(0)), _f(0), True
            else:
                vel = v2[a]
        out['positions'][a], out['angles'][a], out['velocity'][a], out['angvelocity'][a] = pos, angle, vel, spin
        out['slid'][a], out['stopped'][a] = slid, stopped
    return out


def _moved(w, movement):
    """The movement prologue on a copy of the world's velocities: ``movement = (actions (N, A), table (K, 3), keep)``."""
    v, spin = w['velocity'].copy(), w['angvelocity'].copy()
    if movement is not None:
        actions, table, keep = movement
        table = np.asarray(table, _f)
        N, A = spin.shape
        for n in range(N):
            for a in range(A):
                act = int(min(max(actions[n][a], 0), len(table) - 1))
                v[n, a], spin[n, a] = host_move_velocity(keep, w['angles'][n, a], table[act], v[n, a], spin[n, a])
    return v, spin


def slide_rule(w, agent_radius, fps, bounce=.05, movement=None, slide=True):
    """The rule over a world: the seven outputs as (N, A, ..) arrays (``slide=False``: the plain step)."""
    N, A = w['angles'].shape
    v, spin = _moved(w, movement)
    outs = [step_env(w['walls'][n], w['positions'][n], w['angles'][n], v[n], spin[n], agent_radius, fps, bounce, slide) for n in range(N)]
    return {k: np.stack([o[k] for o in outs]) for k in FIELDS}


def plain_scene(w):
    """The oracle's scene of a world's static rows, behind A*4 agent rows an env, which the physics step never reads."""
    A = w['angles'].shape[1]
    rows = [np.concatenate([np.zeros((A*4, 4), _f), x.reshape(-1, 4)]) for x in w['walls']]
    n = sum(map(len, rows))
    return O.Scene(dict(n_agents=A, model=np.zeros((4, 2, 2), _f), lights_vals=np.ones((len(rows), 3), _f), lights_widths=[1]*len(rows),
                        lines_vals=np.concatenate(rows), lines_widths=[len(r) for r in rows], textures_vals=np.ones((n, 3), _f),
                        textures_widths=np.ones(n, np.int32)))


def plain_rule(w, agent_radius, fps, movement=None, scene=None):
    """The plain step by the oracle's own physics: the state and ``progress`` (``scene``: plain_scene(w), made once for a walk)."""
    v, spin = _moved(w, movement)
    ag = dict(positions=w['positions'], angles=w['angles'], velocity=v, angvelocity=spin)
    progress, ag = O.physics(plain_scene(w) if scene is None else scene, ag, O.config(agent_radius, 8, 90., fps))
    return dict({k: ag[k] for k in STATE}, progress=progress)


def host_slide(w, agent_radius, fps, bounce=.05, movement=None, extras=None, raw=False):
    """ms_host_slide over a world, one call. ``extras``: an _lib.MsStepExtras over host arrays the caller keeps alive. Returns the
    seven outputs (``raw``: the call's status instead)."""
    from megastep_amd import _lib
    N, A = w['angles'].shape
    walls = np.ascontiguousarray(np.concatenate([x.reshape(-1, 4) for x in w['walls']] + [np.zeros((1, 4), _f)]), _f)
    starts = np.concatenate([[0], np.cumsum([len(x) for x in w['walls']])]).astype(np.int64)
    st = {k: np.ascontiguousarray(w[k], _f).copy() for k in STATE}
    ag = _lib.MsAgents(st['angles'].ctypes.data, st['positions'].ctypes.data, st['angvelocity'].ctypes.data, st['velocity'].ctypes.data, None, None)
    mv = None
    if movement is not None:
        actions, table = np.ascontiguousarray(movement[0], np.int64), np.ascontiguousarray(movement[1], _f)
        mv = C.byref(_lib.MsMovement(actions.ctypes.data, table.ctypes.data, len(table), float(movement[2])))
    progress, slid, stopped = np.zeros((N, A), _f), np.full((N, A), np.nan, _f), np.full((N, A), 255, np.uint8)
    sl = _lib.MsSlide(float(bounce), slid.ctypes.data, stopped.ctypes.data)
    cfg = _lib.MsConfig(float(agent_radius), 8, 90., float(fps))
    status = _lib.lib().ms_host_slide(walls.ctypes.data, starts.ctypes.data, N, A, C.byref(ag), mv, None if extras is None else C.byref(extras),
                                      C.byref(sl), progress.ctypes.data, C.byref(cfg))
    if raw:
        return status
    assert status == 0, status
    return dict(st, progress=progress, slid=slid, stopped=stopped)


def advance(w, out):
    """The world one step on: ``out``'s state in place of the world's."""
    return dict(walls=w['walls'], **{k: out[k].copy() for k in STATE})


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


ROLLOUT_FIELDS = ('positions', 'angles', 'velocity', 'angvelocity', 'progress', 'stops', 'first_stop', 'trail', 'slides')


def _rollout_buffers(N, A, K, H):
    return dict(positions=np.full((N, A, K, 2), np.nan, _f), angles=np.full((N, A, K), np.nan, _f), velocity=np.full((N, A, K, 2), np.nan, _f),
                angvelocity=np.full((N, A, K), np.nan, _f), progress=np.ones((N, A, K), _f), stops=np.zeros((N, A, K), np.int32),
                first_stop=np.full((N, A, K), H, np.int32), trail=np.full((N, A, K, H, 2), np.nan, _f), slides=np.zeros((N, A, K), np.int32))


def rollout_slide_rule(w, actions, table, keep, others, agent_radius, fps, bounce=.05):
    """The sliding rollouts' rule as a loop over step_env: for every (n, a, k) agent a alone - or, with ``others='rest'``, among
    the env's other agents, at rest where they stand for the whole horizon - stepped H times. ``actions`` (N, A, K, H) or (K, H)."""
    actions, table = np.asarray(actions, np.int64), np.asarray(table, _f)
    N, A = w['angles'].shape
    K, H = actions.shape[-2:]
    out = _rollout_buffers(N, A, K, H)
    for n in range(N):
        for a in range(A):
            who = list(range(A)) if others == 'rest' else [a]
            me = who.index(a)
            for k in range(K):
                plan = actions[k] if actions.ndim == 2 else actions[n, a, k]
                p, ang = w['positions'][n, who].copy(), w['angles'][n, who].copy()
                v, spin = np.zeros((len(who), 2), _f), np.zeros(len(who), _f)
                v[me], spin[me] = w['velocity'][n, a], w['angvelocity'][n, a]
                least, stops, first, slides = _f(1), 0, H, 0
                for h in range(H):
                    act = int(min(max(plan[h], 0), len(table) - 1))
                    v[me], spin[me] = host_move_velocity(keep, ang[me], table[act], v[me], spin[me])
                    o = step_env(w['walls'][n], p, ang, v, spin, agent_radius, fps, bounce)
                    p[me], ang[me], v[me], spin[me] = o['positions'][me], o['angles'][me], o['velocity'][me], o['angvelocity'][me]
                    least = min(least, o['progress'][me])
                    if o['stopped'][me]:
                        stops, first = stops + 1, min(first, h)
                    elif o['slid'][me] > 0:
                        slides += 1
                    out['trail'][n, a, k, h] = p[me]
                out['positions'][n, a, k], out['angles'][n, a, k], out['velocity'][n, a, k], out['angvelocity'][n, a, k] = p[me], ang[me], v[me], spin[me]
                out['progress'][n, a, k], out['stops'][n, a, k], out['first_stop'][n, a, k], out['slides'][n, a, k] = least, stops, first, slides
    return out


def host_rollouts_slide(w, actions, table, keep, others, agent_radius, fps, bounce=.05, raw=False):
    """ms_host_rollouts with slide on, env by env: the nine outputs (``raw``: the first env's status instead)."""
    from megastep_amd import _lib
    actions, table = np.ascontiguousarray(actions, np.int64), np.ascontiguousarray(table, _f)
    N, A = w['angles'].shape
    K, H = actions.shape[-2:]
    out = _rollout_buffers(N, A, K, H)
    cfg = _lib.MsConfig(float(agent_radius), 8, 90., float(fps))
    for n in range(N):
        walls = np.ascontiguousarray(w['walls'][n], _f).reshape(-1, 4)
        st = {k: np.ascontiguousarray(w[k][n], _f) for k in STATE}
        ag = _lib.MsAgents(st['angles'].ctypes.data, st['positions'].ctypes.data, st['angvelocity'].ctypes.data, st['velocity'].ctypes.data, None, None)
        acts = actions if actions.ndim == 2 else np.ascontiguousarray(actions[n])
        env = {k: np.ascontiguousarray(out[k][n]) for k in ROLLOUT_FIELDS}
        r = _lib.MsRollouts(K, H, acts.ctypes.data, int(actions.ndim == 2), table.ctypes.data, len(table), float(keep), int(others == 'rest'), None,
                            *(env[k].ctypes.data for k in ROLLOUT_FIELDS[:8]), 1, float(bounce), env['slides'].ctypes.data)
        status = _lib.lib().ms_host_rollouts(walls.ctypes.data if len(walls) else None, len(walls), C.byref(ag), A, C.byref(r), C.byref(cfg))
        if raw:
            return status
        assert status == 0, status
        for k in ROLLOUT_FIELDS:
            out[k][n] = env[k]
    return out
