"""Items (include/megastep_hip.h, MsItemCollect and MsItemOverlay) restated in numpy - item_rule, one binary32
operation a statement. The collect stands on tests/percept_rule.py's percept_rule (an agent and an item are an eye and a point to
it: the reach test is its in-range statement, the wall test view_rule.blocks); the overlay on a numpy restatement of intersect()
and of the fold raycast_kernel runs over its lines, as the reference writes them (kernels.cu:67-89, 352-377) - without the
division-sparing test ray_fold puts in front, which the equality of the two then covers. Also the host instantiations' harnesses
(ms_host_item_collect, ms_host_item_overlay on numpy arrays) and the worlds the CPU and the GPU suite share."""
import ctypes

import numpy as np

from tests.percept_rule import bits, percept_rule, plan_percepts
from tests.test_navfield_host import F
from tests.test_navview_host import box_walls

NAN, INF = F(np.nan), F(np.inf)
COLLECT_KEYS = ('positions', 'timers', 'taker', 'counts', 'due')
PLANES = ('distances', 'indices', 'locations', 'dots', 'screen')
OVERLAY_KEYS = PLANES + ('items',)


def cross(ax, ay, bx, by):
    m = ax*by
    n = ay*bx
    return m - n


def fold(px, py, rux, ruy, near_s, row, k, f):
    """One line of the reference's fold (kernels.cu:352-377) for arrays of rays: `row` four arrays (or numbers), f the state
    dict(s, idx, t, vx, vy) of arrays, updated in place."""
    with np.errstate(all='ignore'):
        ax, ay, bx, by = (np.broadcast_to(np.asarray(v, F), px.shape) for v in row)
        vx = bx - ax
        vy = by - ay
        uxv = cross(rux, ruy, vx, vy)
        pqx = ax - px
        pqy = ay - py
        s = cross(pqx, pqy, vx, vy)/uxv
        t = cross(pqx, pqy, rux, ruy)/uxv
        flat = ~(np.abs(uxv) >= F(1e-3))                                    # (intersect's early return - and a NaN, which hits nothing)
        s = np.where(flat, INF, s)
        t = np.where(flat, INF, t)
        hit = (0 <= t) & (t <= 1)
        better = (near_s < s) & (s < f['s'] - F(1e-4))
        take = hit & better
    f['s'] = np.where(take, s, f['s'])
    f['idx'] = np.where(take, np.int32(k), f['idx'])
    f['t'] = np.where(take, t, f['t'])
    f['vx'] = np.where(take, vx, f['vx'])
    f['vy'] = np.where(take, vy, f['vy'])


def blank_fold(n):
    return dict(s=np.full(n, INF, F), idx=np.full(n, -1, np.int32), t=np.full(n, NAN, F), vx=np.zeros(n, F), vy=np.zeros(n, F))


def close(rux, ruy, rlen, f):
    """(d, dt) of the fold's winner by raycast_kernel's closing lines (kernels.cu:360-364, 382)."""
    with np.errstate(all='ignore'):
        a = rux*f['vx']
        b = ruy*f['vy']
        dtop = a + b
        a = f['vx']*f['vx']
        b = f['vy']*f['vy']
        vlen = np.sqrt(a + b)
        dbot = rlen*vlen
        dt = dtop/(dbot + F(1e-6))
        d = f['s']*rlen
    return d, dt


def ray_lengths(dirs):
    rux, ruy = np.ascontiguousarray(dirs[..., 0], F), np.ascontiguousarray(dirs[..., 1], F)
    with np.errstate(all='ignore'):
        a = rux*rux
        b = ruy*ruy
        rlen = np.sqrt(a + b)
    return rux, ruy, rlen


def billboard(px, py, cx, cy, radius):
    """The four arrays of the row of an item at c seen from p."""
    with np.errstate(all='ignore'):
        ux = cx - px
        uy = cy - py
        a = ux*ux
        b = uy*uy
        l = np.sqrt(a + b)
        nx = (-uy/l)*F(radius)
        ny = (ux/l)*F(radius)
        return cx - nx, cy - ny, cx + nx, cy + ny


def raycast(walls, origins, dirs, near):
    """The planes of a cast against static walls alone, per env: dict of (N, R) distances, indices (numbered from 0 among `walls`),
    locations, dots - the fold above over the walls in their order."""
    origins, dirs = np.asarray(origins, F), np.asarray(dirs, F)
    N, R = dirs.shape[:2]
    per = R//origins.shape[1]
    out = dict(distances=np.empty((N, R), F), indices=np.empty((N, R), np.int32), locations=np.empty((N, R), F), dots=np.empty((N, R), F))
    for n in range(N):
        px, py = np.repeat(origins[n, :, 0], per), np.repeat(origins[n, :, 1], per)
        rux, ruy, rlen = ray_lengths(dirs[n])
        with np.errstate(all='ignore'):
            near_s = F(near)/rlen
        f = blank_fold(R)
        for l, w in enumerate(np.asarray(walls[n], F).reshape(-1, 4)):
            fold(px, py, rux, ruy, near_s, w, l, f)
        d, dt = close(rux, ruy, rlen, f)
        out['distances'][n], out['indices'][n], out['locations'][n] = d, f['idx'], f['t']
        out['dots'][n] = np.where(f['idx'] >= 0, dt, NAN)
    return out


class item_rule:
    """The contract in numpy: every statement one binary32 operation, in the order the header gives."""

    @staticmethod
    def present(positions):
        return np.isfinite(np.asarray(positions, F)).all(-1)

    @staticmethod
    def collect(walls, agents, positions, timers, kinds, K, reach, delay=0, takers=None, reset=None, through_walls=False):
        """One call of ms_item_collect: dict of the store's positions and timers after it, taker, counts and due; `walls`: a list of
        (L, 4) per env."""
        agents, positions = np.asarray(agents, F), np.array(positions, F)
        timers, kinds = np.array(timers, np.int32), np.asarray(kinds, np.int32)
        (N, A), P = agents.shape[:2], positions.shape[1]
        taker = np.full((N, P), -1, np.int32)
        counts = np.zeros((N, A, K), np.int32)
        for n in range(N):
            if reset is not None and reset[n]:
                positions[n], timers[n] = NAN, 0
                continue
            was = item_rule.present(positions[n])
            best = {}
            for a in range(A):
                if takers is not None and not takers[n][a]:
                    continue
                if through_walls:
                    ok, _, _, rr = percept_rule.candidates(agents[n, a], positions[n], reach)
                else:
                    ok, _, _, rr = percept_rule.visible(walls[n], agents[n, a], positions[n], reach)
                key = np.ascontiguousarray(rr, F).view(np.uint32)
                for k in np.flatnonzero(ok & was):
                    best[k] = min(best.get(k, (2**32, 0)), (int(key[k]), a))
            for k, (_, a) in best.items():
                taker[n, k] = a
                positions[n, k], timers[n, k] = NAN, delay
                if 0 <= kinds[n, k] < K:
                    counts[n, a, kinds[n, k]] += 1
            tick = ~was
            timers[n, tick] = np.where(timers[n, tick] > 0, timers[n, tick] - 1, timers[n, tick])
        due = (~item_rule.present(positions) & (timers == 0)).astype(np.uint8)
        return dict(positions=positions, timers=timers, taker=taker, counts=counts, due=due)

    @staticmethod
    def overlay(positions, colors, origins, dirs, radius, near, lines_widths, planes):
        """One call of ms_item_overlay over `planes` (a dict of some of PLANES, (N, R[, 3]); distances required): the planes after
        it, and items."""
        positions, origins, dirs = np.asarray(positions, F), np.asarray(origins, F), np.asarray(dirs, F)
        (N, R), P = dirs.shape[:2], positions.shape[1]
        per = R//origins.shape[1]
        out = {k: np.array(v) for k, v in planes.items() if v is not None}
        out['items'] = np.full((N, R), -1, np.int32)
        for n in range(N):
            px, py = np.repeat(origins[n, :, 0], per), np.repeat(origins[n, :, 1], per)
            rux, ruy, rlen = ray_lengths(dirs[n])
            with np.errstate(all='ignore'):
                near_s = F(near)/rlen
            f = blank_fold(R)
            for k in range(P):
                fold(px, py, rux, ruy, near_s, billboard(px, py, positions[n, k, 0], positions[n, k, 1], radius), k, f)
            d, dt = close(rux, ruy, rlen, f)
            with np.errstate(all='ignore'):
                wins = (f['idx'] >= 0) & (d < out['distances'][n])
                dn = F(1) - dt*dt
            k = np.where(wins, f['idx'], 0)
            out['items'][n] = np.where(wins, f['idx'], -1)
            out['distances'][n] = np.where(wins, d, out['distances'][n])
            if 'indices' in out:
                out['indices'][n] = np.where(wins, np.int32(lines_widths[n]) + f['idx'], out['indices'][n])
            if 'locations' in out:
                out['locations'][n] = np.where(wins, f['t'], out['locations'][n])
            if 'dots' in out:
                out['dots'][n] = np.where(wins, dt, out['dots'][n])
            if 'screen' in out:
                with np.errstate(all='ignore'):
                    out['screen'][n] = np.where(wins[:, None], dn[:, None]*np.asarray(colors, F)[n, k], out['screen'][n])
        return out


def same(got, want, keys):
    """EQUALITY in every output named: floats by their bits, so that a NaN equals a NaN and nothing else."""
    for key in keys:
        a, b = np.asarray(got[key]), np.asarray(want[key])
        assert a.shape == b.shape and a.dtype == b.dtype, (key, a.shape, b.shape, a.dtype, b.dtype)
        assert np.array_equal(bits(a), bits(b)), (key, int((bits(a) != bits(b)).sum()))


def wall_rows(walls):
    """(rows, starts) as the host instantiations take the static walls: every env's rows, four floats each, 16-byte aligned."""
    rows = np.concatenate([np.asarray(w, F).reshape(-1, 4) for w in walls] + [np.zeros((1, 4), F)])
    starts = np.concatenate([[0], np.cumsum([len(np.asarray(w).reshape(-1, 4)) for w in walls])]).astype(np.int64)
    return np.ascontiguousarray(rows), starts


def host_collect(walls, agents, positions, timers, kinds, K, reach, delay=0, takers=None, reset=None, through_walls=False,
                 fields=('taker', 'counts', 'due'), expect=0):
    """ms_host_item_collect on numpy arrays: the store is copied, the outputs start as sentinels; those not in `fields` are NULL."""
    from megastep_amd import _lib
    agents = np.ascontiguousarray(agents, F)
    (N, A), P = agents.shape[:2], np.asarray(positions).shape[1]
    out = dict(positions=np.ascontiguousarray(positions, F).copy(), timers=np.ascontiguousarray(timers, np.int32).copy(),
               taker=np.full((N, P), -7, np.int32), counts=np.full((N, A, K), -7, np.int32), due=np.full((N, P), 9, np.uint8))
    kinds = np.ascontiguousarray(kinds, np.int32)
    keep = [None if a is None else np.ascontiguousarray(a, np.uint8) for a in (takers, reset)]
    rows, starts = wall_rows(walls)
    ptr = lambda a: None if a is None else a.ctypes.data
    spec = _lib.MsItemCollect(P, K, out['positions'].ctypes.data, out['timers'].ctypes.data, kinds.ctypes.data, ptr(keep[0]), ptr(keep[1]),
                              float(reach), int(delay), int(through_walls), *(ptr(out[k]) if k in fields else None for k in ('taker', 'counts', 'due')))
    status = _lib.lib().ms_host_item_collect(ctypes.byref(spec), N, A, agents.ctypes.data, rows.ctypes.data, starts.ctypes.data)
    assert status == expect
    return out


def host_overlay(positions, colors, origins, dirs, radius, near, lines_widths, planes, items=True, expect=0):
    """ms_host_item_overlay on numpy arrays: the planes given (a dict of some of PLANES) are copied and rewritten; the others NULL."""
    from megastep_amd import _lib
    positions, origins, dirs = (np.ascontiguousarray(a, F) for a in (positions, origins, dirs))
    colors = None if colors is None else np.ascontiguousarray(colors, F)
    (N, R), P, Q = dirs.shape[:2], positions.shape[1], origins.shape[1]
    out = {k: np.ascontiguousarray(v).copy() for k, v in planes.items() if v is not None}
    if items:
        out['items'] = np.full((N, R), -7, np.int32)
    widths = None if lines_widths is None else np.ascontiguousarray(lines_widths, np.int32)
    ptr = lambda a: None if a is None else a.ctypes.data
    spec = _lib.MsItemOverlay(P, R, Q, positions.ctypes.data, ptr(colors), origins.ctypes.data, dirs.ctypes.data, float(radius), float(near),
                              *(ptr(out.get(k)) for k in OVERLAY_KEYS))
    status = _lib.lib().ms_host_item_overlay(ctypes.byref(spec), N, ptr(widths))
    assert status == expect
    return out


# ---------------------------------------------------------------------------------------------------------------------
# worlds
# ---------------------------------------------------------------------------------------------------------------------
class _World:
    pass


_KEPT = {}


def kept(key, make):
    """A world or a rule's result, computed once and shared by the CPU and the GPU suite; never written to."""
    if key not in _KEPT:
        _KEPT[key] = make()
    return _KEPT[key]


def ring(n_rays, phase=0.):
    """(R, 2) directions round the circle, of lengths between a half and two."""
    a = (np.arange(n_rays) + phase)*(2*np.pi/n_rays)
    return (np.stack([np.cos(a), np.sin(a)], -1)*np.linspace(.5, 2., n_rays)[:, None]).astype(F)


def fan(heading, n_rays, fov=130.):
    """(R, 2) directions of a camera-like fan round `heading` (radians)."""
    a = heading + np.radians(np.linspace(-fov/2, fov/2, n_rays)) if n_rays > 1 else np.array([heading])
    return np.stack([np.cos(a), np.sin(a)], -1).astype(F)


def plan_items(P=64, A=3, per=64, seed=31):
    """The six plans of plan_percepts(): A agents an env - its two eyes and points near them - P items from its 200 points (in
    rooms, in walls, hard against them; every seventh absent), kinds of 3, colours, and a fan of `per` rays an agent."""
    def make():
        v = plan_percepts()
        rng = np.random.RandomState(seed + P + 7*A + per)
        w = _World()
        w.walls = v.walls
        w.agents = np.empty((6, A, 2), F)
        for a in range(A):
            w.agents[:, a] = v.eyes[:, a % 2] + (rng.uniform(-.3, .3, (6, 2)) if a >= 2 else 0)
        pick = np.stack([rng.choice(200, P, replace=P > 200) for _ in range(6)])
        w.positions = np.stack([v.points[n][pick[n]] for n in range(6)]).astype(F)
        near = rng.rand(6, P) < .3                                          # (some within an agent's reach)
        w.positions[near] = (w.agents[np.nonzero(near)[0], rng.randint(0, A, near.sum())] + rng.uniform(-.4, .4, (near.sum(), 2))).astype(F)
        w.positions[:, ::7] = NAN
        w.timers = rng.randint(-2, 4, (6, P)).astype(np.int32)
        w.kinds = rng.randint(0, 3, (6, P)).astype(np.int32)
        w.colors = rng.uniform(0, 1, (6, P, 3)).astype(F)
        w.dirs = np.stack([np.concatenate([fan(rng.uniform(0, 2*np.pi), per) for _ in range(A)]) for _ in range(6)])
        w.widths = np.array([len(x) + A*2 for x in w.walls], np.int32)
        return w
    return kept(('plan', P, A, per, seed), make)


def hand_items(P, A, seed=0):
    """One env of box_walls() - the 8 x 4 box, its partition with a door, its NaN row - with A agents and P items drawn in and a
    little beyond the box, a third of the items within a step of some agent, every fifth absent."""
    def make():
        rng = np.random.RandomState(1000*A + P + seed)
        w = _World()
        w.walls = [box_walls()]
        w.agents = rng.uniform((.2, .2), (7.8, 3.8), (1, A, 2)).astype(F)
        w.positions = rng.uniform((-.5, -.5), (8.5, 4.5), (1, P, 2)).astype(F)
        near = rng.rand(P) < .34
        w.positions[0, near] = (w.agents[0, rng.randint(0, A, near.sum())] + rng.uniform(-.3, .3, (near.sum(), 2))).astype(F)
        w.positions[0, 3::5] = NAN
        w.timers = rng.randint(-2, 4, (1, P)).astype(np.int32)
        w.kinds = rng.randint(0, 8, (1, P)).astype(np.int32)
        w.colors = rng.uniform(0, 1, (1, P, 3)).astype(F)
        w.takers = (rng.rand(1, A) < .8).astype(np.uint8)
        w.widths = np.array([len(w.walls[0]) + 2*A], np.int32)
        return w
    return kept(('hand', P, A, seed), make)


WIDE_SETS = ('sprinkled', 'late', 'full', 'on')
OVERLAY_WINDOW = 256                                                        # item_overlay_kernel's WG: items a window, rays a chunk
WIDE_RADIUS = .03                                                           # billboards thin enough that rays pass between a thousand


def wide_items(P, which, A=3):
    """hand_items(P, A) with more items than one window of item_overlay_kernel's compaction holds, present as `which` says:
    'sprinkled' every fifth absent, as hand_items() has them; 'late' the first window's 256 all absent and every later one present;
    'full' every item present; 'on' as 'sprinkled', with item 1 exactly on agent 0 and item 256 exactly on agent 1 (a NaN billboard
    for that origin alone)."""
    def make():
        base = hand_items(P, A)
        rng = np.random.RandomState(77 + P)
        w = _World()
        w.__dict__.update(base.__dict__)
        w.positions = base.positions.copy()
        if which in ('late', 'full'):
            absent = np.isnan(w.positions[0, :, 0])
            w.positions[0, absent] = rng.uniform((-.5, -.5), (8.5, 4.5), (absent.sum(), 2)).astype(F)
        if which == 'late':
            w.positions[0, :OVERLAY_WINDOW] = NAN
        if which == 'on':
            w.positions[0, 1], w.positions[0, OVERLAY_WINDOW] = base.agents[0, 0], base.agents[0, 1]
        return w
    assert which in WIDE_SETS and P > OVERLAY_WINDOW
    return kept(('wide', P, which, A), make)


def overlay_windows(positions, origin):
    """The live billboards (no NaN: the item present and not exactly at `origin`) one origin keeps of an env's items ((P, 2)) in
    each window of item_overlay_kernel's compaction, in the kernel's order; their sum is the `kept` its rays fold over."""
    positions = np.asarray(positions, F)
    live = ~np.isnan(positions).any(-1) & ~(positions == np.asarray(origin, F)).all(-1)
    return [int(live[k0:k0 + OVERLAY_WINDOW].sum()) for k0 in range(0, len(live), OVERLAY_WINDOW)]


def check_wide(w, which):
    """The counted facts of wide_items(P, which), origin by origin: what each set is there to put the kernel through."""
    P = w.positions.shape[1]
    for a, origin in enumerate(w.agents[0]):
        wins = overlay_windows(w.positions[0], origin)
        assert len(wins) == -(-P//OVERLAY_WINDOW) >= 2
        if which == 'sprinkled':
            assert wins[0] % 64 and wins[0] < OVERLAY_WINDOW and all(wins), wins     # (the second window starts inside a wave's 64)
        elif which == 'late':
            assert wins[0] == 0 and all(wins[1:]) and sum(wins) == P - OVERLAY_WINDOW, wins
        elif which == 'full':
            assert sum(wins) == P, wins                                               # (P = 1024: the last slot of the LDS is written)
        else:
            plain = overlay_windows(hand_items(P, w.agents.shape[1]).positions[0], origin)
            assert [x - y for x, y in zip(plain, wins)] == [[1, 0], [0, 1], [0, 0]][a] + [0]*(len(wins) - 2), (plain, wins)


def wall_planes(walls, origins, dirs, near, widths, offset):
    """The planes a cast against the static walls leaves, numbered as the device numbers an env's lines (the agents' rows first:
    `offset` of them), with a screen of a flat grey where something was hit."""
    def make():
        base = raycast(walls, origins, dirs, near)
        base['indices'] = np.where(base['indices'] >= 0, base['indices'] + np.int32(offset), base['indices']).astype(np.int32)
        base['screen'] = np.where((base['indices'] >= 0)[..., None], F(.25), F(0)).astype(F)*np.ones(3, F)
        return base
    return make()
