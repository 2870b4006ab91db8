"""Sliding walkers (include/megastep_hip.h, MsWalkers with slide) in numpy - walk_slide_rule: walker_rule's steer, apart
and blend as they stand, then the agents' contact rule (slide_rule's normals and order) around the oracle's own collision_cc and
collision_cs with no cull in front, one binary32 operation a statement - and ms_host_walkers with the new fields on arrays."""
import numpy as np

from tests import walker_rule as wr
from tests.slide_rule import _less, _normal_agent, _normal_wall
from tests.walker_rule import F, NAN, RADIUS, _cc, _cs

KEYS = wr.KEYS + ('slid', 'stopped')


def _free(walls, agents, store, towards, **kw):
    """walk_rule's steps 1 to 4: its tick with nothing to meet stores every walker's v of the tick - and counts `close`."""
    cc, wr._cc = wr._cc, lambda *a: F(1)
    try:
        return wr.walk_rule([np.zeros((0, 4), F) for _ in walls], agents, store, towards, **kw)
    finally:
        wr._cc = cc


def walk_slide_rule(walls, agents, store, towards, personal=.6, push=1., keep=.5, agents_push=True, reset=None, fps=10., radius=RADIUS,
                    bounce=.05, slide=True, steps=None):
    """One tick: the store after it and the records. `steps`: a list that takes (x0, y0, x1, y1) of every move, phase A's and phase B's.
    `slide=False`: every blocked walker stops dead - the plain tick by these statements."""
    agents = np.asarray(agents, F)
    (N, A), P = agents.shape[:2], store['positions'].shape[1]
    free = _free(walls, agents, store, towards, personal=personal, push=push, keep=keep, agents_push=agents_push, reset=reset, fps=fps, radius=radius)
    fps, radius, bounce, one, zero = F(fps), F(radius), F(bounce), F(1), np.zeros(2, F)
    out = {k: np.array(store[k]) for k in wr.STORE}
    out.update(progress=np.full((N, P), NAN, F), blocked=np.full((N, P), 4, np.uint8), bumps=np.zeros((N, A), np.int32), close=free['close'],
               slid=np.full((N, P), NAN, F), stopped=np.full((N, P), 4, np.uint8))
    with np.errstate(all='ignore'):
        for n in range(N):
            if reset is not None and reset[n]:
                out['positions'][n] = NAN
                continue
            pos, v = np.array(store['positions'][n], F), free['velocities'][n]
            there = np.isfinite(pos).all(-1)
            u, rows = v/fps, np.asarray(walls[n], F).reshape(-1, 4)
            at_rest = [(agents[n, a], a) for a in range(A) if np.isfinite(agents[n, a]).all()]
            p1, v2, u2, r1, slides = pos.copy(), v.copy(), np.zeros((P, 2), F), np.zeros(P, F), np.zeros(P, bool)
            for k in np.flatnonzero(there):                                                   # phase A and the contact
                met = []                                                                      # (c, class, its normal at a point)
                for o, a in at_rest:
                    c = _cc(pos[k], u[k], o, zero, radius)
                    out['bumps'][n, a] += c < 1
                    met.append((c, 1, lambda p, o=o, c=c: _normal_agent(p, o, zero, c)))
                for j in np.flatnonzero(there):
                    if j != k:
                        c = _cc(pos[k], u[k], pos[j], u[j], radius)
                        met.append((c, 2, lambda p, j=j, c=c: _normal_agent(p, pos[j], u[j], c)))
                for row in rows:
                    met.append((_cs(pos[k], u[k], row, radius), 3, lambda p, row=row: _normal_wall(p, row)))
                x1, cls = min([(c, cls) for c, cls, _ in met if c < 1] + [(one, 0)])
                p1[k] = pos[k] + F(x1*v[k])/fps
                out['progress'][n, k], out['blocked'][n, k] = x1, cls
                best = None
                for c, _, normal in met if slide and x1 < 1 else ():
                    nrm = normal(p1[k]) if c == x1 else None
                    if nrm is not None:
                        key = (F(F(v[k, 0]*nrm[0]) + F(v[k, 1]*nrm[1])), nrm[0], nrm[1])
                        best = key if _less(key, best) else best
                if best is not None and best[0] < 0:
                    slides[k], r1[k], f = True, F(one - x1), F(F(one + bounce)*best[0])
                    v2[k] = (F(v[k, 0] - F(f*best[1])), F(v[k, 1] - F(f*best[2])))
                    u2[k] = F(v2[k]*r1[k])/fps
            for k in np.flatnonzero(there):                                                   # phase B: the others as phase A left them
                new, vel, slid, stopped = p1[k], v[k], F(0), out['progress'][n, k] < 1
                if slides[k]:
                    xs = [_cc(p1[k], u2[k], o, zero, radius) for o, _ in at_rest]
                    xs += [_cc(p1[k], u2[k], p1[j], u2[j], radius) for j in np.flatnonzero(there) if j != k]
                    xs += [_cs(p1[k], u2[k], row, radius) for row in rows]
                    x2 = one
                    for c in xs:
                        x2 = c if c < x2 else x2
                    new, vel, slid, stopped = p1[k] + F(x2*u2[k]), v2[k], F(x2*r1[k]), x2 < 1
                if steps is not None:
                    steps += [(*pos[k], *p1[k]), (*p1[k], *new)]
                out['positions'][n, k], out['velocities'][n, k] = new, (zero if stopped else vel)
                out['slid'][n, k], out['stopped'][n, k] = slid, stopped
    return out


def host_walk_slide(walls, agents, store, towards, bounce=.05, slide=1, expect=0, spoil=(), **kw):
    """ms_host_walkers with the new fields set. `spoil` as host_walk's, applied behind them."""
    N, P = store['positions'].shape[:2]
    slid, stopped = np.full((N, P), 7, F), np.full((N, P), 9, np.uint8)
    fields = (('slide', slide), ('bounce', float(bounce)), ('slid', slid.ctypes.data), ('stopped', stopped.ctypes.data))
    return dict(wr.host_walk(walls, agents, store, towards, expect=expect, spoil=fields + tuple(spoil), **kw), slid=slid, stopped=stopped)
