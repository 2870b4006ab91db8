"""Percepts (include/megastep_hip.h, MsPercepts) restated in numpy - percept_rule, one binary32 operation a
statement - on tests/test_navview_host.py's view_rule: a pair of an eye and a point is a viewpoint and a cell centre to
view_rule.blocks, and the in-range and in-cone statements are view_rule's, written for a point in place of a grid's centres. The
nearest go by a Python sort of (bits of rr, p). Also the host instantiation's harness (ms_host_percepts on numpy arrays) and the
worlds the CPU and the GPU suite share."""
import ctypes

import numpy as np

from tests.test_navfield_host import F
from tests.test_navview_host import CONE, box_walls, cos_half_of, plan_views, view_rule

KEYS = ('visible', 'squares', 'offsets', 'counts', 'nearest', 'near_offsets', 'near_distances')
NAN, INF = F(np.nan), F(np.inf)


class percept_rule:
    """The contract in numpy: every statement one binary32 operation, in the order the header gives."""

    @staticmethod
    def eye(p, heading):
        """Does view_point accept the eye: (live, hlen)."""
        px, py = F(p[0]), F(p[1])
        if not (np.isfinite(px) and np.isfinite(py)):
            return False, F(0)
        if heading is None:
            return True, F(0)
        hx, hy = F(heading[0]), F(heading[1])
        with np.errstate(all='ignore'):
            a = hx*hx
            b = hy*hy
            hlen = np.sqrt(F(a + b))
        return bool(np.isfinite(hlen) and hlen > 0), hlen

    @staticmethod
    def candidates(p, points, R, heading=None, cos_half=None):
        """((P,) bool, rx, ry, rr): view_candidate of every point - view_rule.in_range's and in_cone's statements."""
        x, y = np.asarray(points, F)[:, 0], np.asarray(points, F)[:, 1]
        live, hlen = percept_rule.eye(p, heading)
        px, py = F(p[0]), F(p[1])
        with np.errstate(all='ignore'):
            R2 = F(R)*F(R)
            rx = x - px
            ry = y - py
            a = rx*rx
            b = ry*ry
            rr = a + b
            ok = rr <= R2
            if heading is not None:
                hx, hy = F(heading[0]), F(heading[1])
                length = np.sqrt(rr)
                a = hx*rx
                b = hy*ry
                dotp = a + b
                lim = F(cos_half)*length
                lim = lim*hlen
                ok = ok & (dotp >= lim)
        return (ok if live else np.zeros(len(x), bool)), rx, ry, rr

    @staticmethod
    def visible(walls, p, points, R, heading=None, cos_half=None, wanted=None):
        """((P,) bool, rx, ry, rr): the points in sight of the eye p."""
        ok, rx, ry, rr = percept_rule.candidates(p, points, R, heading, cos_half)
        if wanted is not None:
            ok = ok & wanted
        walls = np.asarray(walls, F).reshape(-1, 4)
        if ok.any() and len(walls):
            at = np.flatnonzero(ok)
            pts = np.asarray(points, F)
            blocked = np.zeros(len(at), bool)
            for first in range(0, len(walls), 64):
                blocked |= view_rule.blocks(p[0], p[1], pts[at, 0], pts[at, 1], walls[first:first + 64]).any(1)
            ok = ok.copy()
            ok[at] = ~blocked
        return ok, rx, ry, rr

    @staticmethod
    def call(walls, eyes, points, R, K, headings=None, cos_half=None, valid=None, pairs=None, mask=None, before=None):
        """One call of ms_percepts: dict of the seven outputs; `walls`: a list of (L, 4) per env; `before`: what the outputs held (the
        rows of masked-out eyes keep it)."""
        eyes, points = np.asarray(eyes, F), np.asarray(points, F)
        (N, E), P = eyes.shape[:2], points.shape[1]
        out = before if before is not None else blank(N, E, P, K)
        out = {k: np.array(v) for k, v in out.items()}
        for n in range(N):
            for e in range(E):
                if mask is not None and not mask[n][e]:
                    continue
                wanted = np.ones(P, bool)
                if valid is not None:
                    wanted &= np.asarray(valid[n]) != 0
                if pairs is not None:
                    wanted &= np.asarray(pairs[n][e] if np.ndim(pairs) == 3 else pairs[e]) != 0
                vis, rx, ry, rr = percept_rule.visible(walls[n], eyes[n, e], points[n], R, None if headings is None else headings[n, e], cos_half, wanted)
                out['visible'][n, e] = vis
                out['squares'][n, e] = np.where(vis, rr, INF)
                out['offsets'][n, e, :, 0] = np.where(vis, rx, NAN)
                out['offsets'][n, e, :, 1] = np.where(vis, ry, NAN)
                out['counts'][n, e] = vis.sum()
                bits = np.ascontiguousarray(rr, F).view(np.uint32)
                order = [p for _, p in sorted((int(bits[p]), int(p)) for p in np.flatnonzero(vis))][:K]
                out['nearest'][n, e] = -1
                out['near_offsets'][n, e] = NAN
                out['near_distances'][n, e] = INF
                for k, p in enumerate(order):
                    out['nearest'][n, e, k] = p
                    out['near_offsets'][n, e, k] = (rx[p], ry[p])
                    with np.errstate(all='ignore'):
                        out['near_distances'][n, e, k] = np.sqrt(rr[p])
        return out


def blank(N, E, P, K):
    """The seven outputs holding sentinels no call writes."""
    return dict(visible=np.full((N, E, P), 9, np.uint8), squares=np.full((N, E, P), -7, F), offsets=np.full((N, E, P, 2), -7, F),
                counts=np.full((N, E), -7, np.int32), nearest=np.full((N, E, K), -7, np.int32), near_offsets=np.full((N, E, K, 2), -7, F),
                near_distances=np.full((N, E, K), -7, F))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(got, want, keys=KEYS):
    """EQUALITY in every output named: floats by their bits, so that a NaN equals a NaN and nothing else."""
    for key in keys:
        a, b = np.asarray(got[key]), np.asarray(want[key])
        assert a.shape == b.shape and a.dtype == b.dtype, (key, a.shape, b.shape, a.dtype, b.dtype)
        assert np.array_equal(bits(a), bits(b)), (key, int((bits(a) != bits(b)).sum()))


def host(walls, eyes, points, R, K, headings=None, cos_half=0., valid=None, pairs=None, mask=None, before=None, capacity=0, fields=KEYS,
         expect=0):
    """ms_host_percepts on numpy arrays; the outputs start as `before` (default: sentinels); those not in `fields` are passed as NULL."""
    from megastep_amd import _lib
    eyes, points = np.ascontiguousarray(eyes, F), np.ascontiguousarray(points, F)
    (N, E), P = eyes.shape[:2], points.shape[1]
    out = before if before is not None else blank(N, E, P, K)
    out = {k: np.ascontiguousarray(v).copy() for k, v in out.items()}
    rows = np.ascontiguousarray(np.concatenate([np.asarray(w, F).reshape(-1, 4) for w in walls] + [np.zeros((1, 4), F)]))
    starts = np.concatenate([[0], np.cumsum([len(np.asarray(w).reshape(-1, 4)) for w in walls])]).astype(np.int64)
    keep = [None if a is None else np.ascontiguousarray(a, t) for a, t in ((headings, F), (valid, np.uint8), (pairs, np.uint8), (mask, np.uint8))]
    ptr = lambda a: None if a is None or a.size == 0 else a.ctypes.data
    spec = _lib.MsPercepts(E, P, K, eyes.ctypes.data, ptr(keep[0]), points.ctypes.data, ptr(keep[1]), ptr(keep[2]),
                           0 if pairs is None else 1 if keep[2].ndim == 2 else 2, ptr(keep[3]), float(R), float(cos_half),
                           *(ptr(out[k]) if k in fields else None for k in KEYS))
    status = _lib.lib().ms_host_percepts(ctypes.byref(spec), N, rows.ctypes.data, starts.ctypes.data, capacity)
    assert status == expect
    return out


class _World:
    pass


_PLANS = []


def plan_percepts():
    """The six plans of plan_views() with its two viewpoints a plan as eyes, its headings, and 200 points a plan from
    RandomState(21), uniform in the bounding box of the plan's walls - in rooms, in walls, hard against them."""
    if not _PLANS:
        v = plan_views()
        w = _World()
        w.walls, w.eyes, w.headings, w.cos_half = v.walls, v.points, v.headings, v.cos_half
        rng = np.random.RandomState(21)
        w.points = np.empty((6, 200, 2), F)
        for n in range(6):
            ends = np.concatenate([v.walls[n][:, :2], v.walls[n][:, 2:]])
            w.points[n] = rng.uniform(ends.min(0), ends.max(0), (200, 2)).astype(F)
        w.rule = {}
        _PLANS.append(w)
    return _PLANS[0]


def plan_rule(R, cone, K):
    """percept_rule.call on plan_percepts(), kept: the CPU and the GPU suite compare against the same arrays."""
    w = plan_percepts()
    if (R, cone, K) not in w.rule:
        kw = dict(headings=w.headings, cos_half=w.cos_half) if cone else {}
        w.rule[R, cone, K] = percept_rule.call(w.walls, w.eyes, w.points, R, K, **kw)
    return w.rule[R, cone, K]


_HAND = {}


def hand_shape(E, P, seed=0):
    """One env of box_walls() - the 8 x 4 box, its partition with a door, its NaN row - with E eyes and P points drawn in and a
    little beyond the box, headings of any length, and a valid and a pairs tensor that switch a few off."""
    if (E, P, seed) not in _HAND:
        rng = np.random.RandomState(100*E + P + seed)
        w = _World()
        w.walls = [box_walls()]
        w.eyes = rng.uniform((.2, .2), (7.8, 3.8), (1, E, 2)).astype(F)
        w.points = rng.uniform((-.5, -.5), (8.5, 4.5), (1, P, 2)).astype(F)
        w.headings = (rng.uniform(-1, 1, (1, E, 2))*rng.choice([.5, 3.], (1, E, 1))).astype(F)
        w.valid = (rng.rand(1, P) < .9).astype(np.uint8)
        w.pairs = (rng.rand(E, P) < .9).astype(np.uint8)
        w.cos_half = cos_half_of(CONE)
        _HAND[E, P, seed] = w
    return _HAND[E, P, seed]
