"""Constructions for the step kernels' device-only text and their counted facts, in plain numpy plus the host hooks -
no GPU here: tests/test_step_edges_host.py asserts the counts, tests/test_gpu_step_edges.py imports the same constructions and
the same counts and runs them.

Action tables of any size with pairwise distinct rows, and the actions that must appear in every call; the wild actions; and
the rosette - short walls on a ring round a tight cluster of agents that all move alike, plus a frame far away - whose (wall, agent)
pairs are each well inside the agents' reach or well outside it, so that how many pairs each LDS list receives, window by window
in the kernel's own order, is a matter of counting. The models below restate the kernels' list bookkeeping (when a list is
flushed, how full it gets); their thresholds are read out of the sources by constants()."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
FPS = 10.
RADIUS = 1/2**.5*.15                                                     # core.AGENT_RADIUS

WAVE = 64
TABLE_SIZES = (1, 7, 21, 22, 64)                                         # 21: the last table held in a register's lanes; 22: the first read from memory


def constants():
    """The kernels' own thresholds, read out of their sources."""
    def grab(path, name):
        text = open(os.path.join(ROOT, 'megastep_amd', 'csrc', 'kernels', path)).read()
        m = re.search(r'constexpr int %s = ([^;]+);' % name, text)
        assert m, name
        return m.group(1)
    ahead, few = int(grab('physics.h', 'PHYS_AHEAD')), int(grab('physics.h', 'PHYS_FEW'))
    assert grab('physics.h', 'PHYS_PAIRS') == '(PHYS_FEW + 1)*WAVE' and grab('rollout.h', 'ROLL_PAIRS') == '4*WAVE'
    return dict(PHYS_AHEAD=ahead, PHYS_FEW=few, PHYS_PAIRS=(few + 1)*WAVE, ROLL_PAIRS=4*WAVE, ROLL_AHEAD=int(grab('step.h', 'ROLL_AHEAD')),
                ROLL_FEW=int(grab('rollout.h', 'ROLL_FEW')))


PHYS_AHEAD, PHYS_FEW, PHYS_PAIRS, ROLL_PAIRS, ROLL_AHEAD, ROLL_FEW = 4, 4, 320, 256, 4, 24


# ---------------------------------------------------------------------------------------------------------------------
# tables and actions
# ---------------------------------------------------------------------------------------------------------------------
def table(T, turning=True):
    """(T, 3) float32, rows pairwise distinct: row 0 the no-op (the chained references give it to agents at rest); row i moves at
    3 .. 4 m/s along a direction of its own; with `turning` every fifth row also turns, by +-30 degrees a second."""
    i = np.arange(T)
    a = 2.399963*i
    speed = 3. + ((7*i) % max(T, 2))/max(T, 2)
    t = np.stack([speed*np.cos(a), speed*np.sin(a), np.where((i % 5 == 4) & turning, 30.*(-1.)**i, 0.)], -1).astype(F)
    t[0] = 0.
    assert len({r.tobytes() for r in t}) == T
    return t


def must_rows(T):
    """The rows every call's actions include: the first, the last, and the two either side of the register's last lane."""
    return sorted({0, T - 1} | {r for r in (20, 21) if r < T})


def actions(shape, T, seed=0):
    """int64 actions of `shape` in [0, T), with must_rows(T) among the first elements."""
    a = np.random.RandomState(seed).randint(0, T, shape).astype(np.int64)
    must = must_rows(T)
    assert a.size >= len(must)
    a.reshape(-1)[:len(must)] = must
    return a


def wild_values(T):
    """Actions outside a table of T rows. 2**32 + 3 narrows to the valid row 3: it tells clamp-then-narrow from narrow-then-clamp."""
    return [-2**63, -2**40, -1, T, T + 1, 2**31, 2**32 + 3, 2**63 - 1]


def wild(a, T):
    """`a` (from actions()) with every wild value once, behind the rows that must appear; and the clamped tensor it must equal.
    Valid rows stay among them."""
    a = a.copy()
    flat, must, vals = a.reshape(-1), len(must_rows(T)), wild_values(T)
    assert flat.size > must + len(vals)
    flat[must:must + len(vals)] = vals
    want = np.clip(a, 0, T - 1)
    narrowed = np.clip(a.astype(np.int32), 0, T - 1).astype(np.int64)  # (what narrowing first would make of them)
    assert (narrowed != want).any() and ((a >= 0) & (a < T)).any()
    return a, want, narrowed


# ---------------------------------------------------------------------------------------------------------------------
# the host hooks
# ---------------------------------------------------------------------------------------------------------------------
def _fp(x):
    return x.ctypes.data_as(C.POINTER(C.c_float))


def task_of(position, velocity):
    """(x, y, ux, uy): an agent's task as the kernels form it, u = v/fps in binary32."""
    return np.array([position[0], position[1], F(velocity[0])/F(FPS), F(velocity[1])/F(FPS)], F)


def reach_of(task):
    from megastep_amd import _lib
    return F(_lib.lib().ms_host_wall_reach(_fp(np.ascontiguousarray(task, F)), float(RADIUS)))


def beyond(task, row):
    """ms_host_wall_beyond_reach: is the row beyond the task's reach (the cull in front of the exact test)?"""
    from megastep_amd import _lib
    return bool(_lib.lib().ms_host_wall_beyond_reach(_fp(np.ascontiguousarray(task, F)), _fp(np.ascontiguousarray(row, F)), float(RADIUS)))


def distance(point, row):
    """From a point to the nearest point of the segment `row`, in float64."""
    p, a, b = np.asarray(point[:2], float), np.asarray(row[:2], float), np.asarray(row[2:], float)
    v = b - a
    t = np.clip(np.dot(p - a, v)/max(np.dot(v, v), 1e-300), 0, 1)
    return float(np.hypot(*(a + t*v - p)))


def in_reach(tasks, rows):
    """(A, W) bool: the host's verdict pair by pair - and every pair's margin asserted: a row in reach is nearer than half the
    reach, one beyond it farther than twice (odd rows - a NaN, or shorter than 1e-4 m - are never beyond, at any distance)."""
    out = np.zeros((len(tasks), len(rows)), bool)
    for t, task in enumerate(tasks):
        reach = float(reach_of(task))
        for l, row in enumerate(rows):
            out[t, l] = not beyond(task, row)
            if not odd_rows(row[None])[0]:
                d = distance(task, row)
                assert (d < .5*reach) if out[t, l] else (d > 2*reach), (t, l, d, reach)
            else:
                assert out[t, l]
    return out


def odd_rows(rows):
    """physics_kernel's `odd`: a coordinate that is not finite, or a row shorter than 1e-4 m - kept whatever the boxes say."""
    rows = np.asarray(rows, F)
    with np.errstate(invalid='ignore'):
        dx, dy = rows[:, 2] - rows[:, 0], rows[:, 3] - rows[:, 1]
        return ~np.isfinite(rows).all(1) | ~(dx*dx + dy*dy >= F(1e-8))


def boxes_touch(tasks, rows):
    """(A, W) bool: does the row's bounding box touch the agent's reach box - the sweep's test, in the kernel's own binary32
    compares - with every verdict's margin asserted: the boxes overlap by, or are apart by, more than a centimetre."""
    rows = np.asarray(rows, F)
    with np.errstate(invalid='ignore'):
        x0, x1 = np.fmin(rows[:, 0], rows[:, 2]), np.fmax(rows[:, 0], rows[:, 2])
        y0, y1 = np.fmin(rows[:, 1], rows[:, 3]), np.fmax(rows[:, 1], rows[:, 3])
        out = np.zeros((len(tasks), len(rows)), bool)
        for t, task in enumerate(tasks):
            reach = reach_of(task)
            bx0, by0, bx1, by1 = task[0] - reach, task[1] - reach, task[0] + reach, task[1] + reach
            away = (x1 < bx0) | (x0 > bx1) | (y1 < by0) | (y0 > by1)
            gap = np.maximum.reduce([bx0 - x1, x0 - bx1, by0 - y1, y0 - by1])       # > 0: apart by that much; < 0: overlapping
            assert (np.abs(gap[np.isfinite(gap)]) > .01).all(), t
            out[t] = ~away
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the rosette
# ---------------------------------------------------------------------------------------------------------------------
class Rosette:
    """One env: `order` names its static rows in their order - 'r' a short wall on the ring (radius .18) round cluster 0 at (6, 6),
    's' one on the ring round cluster 1 at (9, 3), 'f' one of the frame's four (the 12 m square: far from everybody), 'n' a ring
    wall of cluster 0 with a NaN coordinate, 't' one shorter than 1e-4 m; `homes`: which cluster each agent belongs to - it sits
    within 5 cm of the centre; `gap`: the third of ring 0 round this direction (degrees) is left open."""
    CENTRES = np.array([[6., 6.], [9., 3.]])
    RING = .18
    FRAME = np.array([[0, 0, 12, 0], [12, 0, 12, 12], [12, 12, 0, 12], [0, 12, 0, 0]], F)

    def __init__(self, order, homes, gap=180., seed=0):
        self.order, self.homes = order, list(homes)
        rng = np.random.RandomState(seed)
        per = [sum(k in kinds for k in order) for kinds in ('rnt', 's')]
        seen, frame, rows = [0, 0], 0, []
        for k in order:
            if k == 'f':
                rows.append(self.FRAME[frame % 4]); frame += 1
                continue
            c = 1 if k == 's' else 0
            arc = 240. if c == 0 else 360.
            a = np.radians(gap + 60. + arc*(seen[c] + .5)/per[c]) if c == 0 else 2*np.pi*seen[c]/per[c]
            seen[c] += 1
            half = min(.4*np.radians(arc)*self.RING/per[c], .025) if k != 't' else 2e-5
            mid, tangent = self.CENTRES[c] + self.RING*np.array([np.cos(a), np.sin(a)]), np.array([-np.sin(a), np.cos(a)])
            row = np.concatenate([mid - half*tangent, mid + half*tangent]).astype(F)
            if k == 'n':
                row[2] = np.nan
            rows.append(row)
        self.rows = np.stack(rows).astype(F)
        spread = rng.uniform(-.035, .035, (len(self.homes), 2))
        self.positions = (self.CENTRES[self.homes] + spread).astype(F)
        assert len({p.tobytes() for p in self.positions}) == len(self.positions)

    @property
    def walls(self):
        """(W, 2, 2) float64 for scene.scenery (binary32 values: they come back as the rows they are)."""
        return self.rows.astype(float).reshape(-1, 2, 2)

    def velocity(self, heading, speed=4.):
        """Everybody at `speed` m/s along `heading` (degrees): agents that move alike never meet each other."""
        a = np.radians(heading)
        return np.tile(np.array([speed*np.cos(a), speed*np.sin(a)], F), (len(self.homes), 1))

    def tasks(self, heading, speed=4.):
        return [task_of(p, v) for p, v in zip(self.positions, self.velocity(heading, speed))]


# ---------------------------------------------------------------------------------------------------------------------
# the kernels' list bookkeeping
# ---------------------------------------------------------------------------------------------------------------------
def sweep_trace(touch, odd):
    """physics_kernel's sweep without a grid over W static rows: touch (A, W) from boxes_touch(), odd (W,). One entry per 64-row
    window, in the kernel's order: (branch, pairs in the list behind the window, flushes inside it); and the list's peak. (A window
    of fewer than 64 rows - the env's last - always takes the other branch: the lanes past the last row hold zeros, a row of no
    length, which the kernel's `odd` ballot counts before `live` masks it.)"""
    A, W = touch.shape
    few = A <= PHYS_FEW
    cnt, peak, trace = 0, 0, []
    for w0 in range(0, W, WAVE):
        win = slice(w0, w0 + WAVE)
        flushes = 0
        if few and not odd[win].any() and w0 + WAVE <= W:
            n = int(touch[:, win].sum())
            if n:
                if cnt > PHYS_PAIRS - PHYS_FEW*WAVE:
                    cnt, flushes = 0, 1
                cnt += n
            branch = 'few'
        else:
            for t in range(A):
                if cnt > PHYS_PAIRS - WAVE:
                    cnt, flushes = 0, flushes + 1
                cnt += int((touch[t, win] | odd[win]).sum())
                peak = max(peak, cnt)
            branch = 'each'
        peak = max(peak, cnt)
        assert peak <= PHYS_PAIRS
        trace.append((branch, cnt, flushes))
    return trace, peak


def rounds(W):
    """How many rounds of PHYS_AHEAD x 64 rows the sweep's outer loop takes over W static rows."""
    return -(-W//(PHYS_AHEAD*WAVE))


def list_trace(kept, cap):
    """A PairList of `cap` slots fed windows of up to 64 lanes, `kept` of them appended each: the list's length behind every
    window (0 behind a window that found it too full and flushed first... then `kept`), the number of flushes, the peak."""
    cnt, peak, flushes, lengths = 0, 0, 0, []
    for k in kept:
        assert 0 <= k <= WAVE
        if cnt > cap - WAVE:
            cnt, flushes = 0, flushes + 1
        cnt += int(k)
        peak = max(peak, cnt)
        lengths.append(cnt)
    assert peak <= cap
    return lengths, flushes, peak


def deal_windows(counts, verdicts):
    """The gridded deal: the agents' near lists (`counts` rows each; `verdicts`: one bool array per agent - is the row in reach)
    laid end to end and dealt 64 pairs a window. Returns P and the pairs kept in each window."""
    flat = np.concatenate([np.asarray(v, bool)[:c] for c, v in zip(counts, verdicts)]) if sum(counts) else np.zeros(0, bool)
    P = int(sum(counts))
    assert len(flat) == P
    return P, [int(flat[p0:p0 + WAVE].sum()) for p0 in range(0, P, WAVE)]


def rollout_windows(verdicts):
    """rollout_walls_kernel at one step: candidate after candidate, each one's rows (`verdicts`: one bool array per candidate) in
    windows of 64. The pairs kept in each window, in the kernel's order."""
    return [int(np.asarray(v, bool)[j0:j0 + WAVE].sum()) for v in verdicts for j0 in range(0, len(v), WAVE)]


# ---------------------------------------------------------------------------------------------------------------------
# the constructions, by name: what the GPU module runs and what the CPU module counts
# ---------------------------------------------------------------------------------------------------------------------
SWEEPS = {
    # physics_kernel, no grid, five agents (beyond PHYS_FEW): every agent's box touches every ring wall
    'each-full': dict(order='r'*64 + 'f'*4, homes=[0]*5, trace=[('each', 320, 0), ('each', 0, 1)], peak=320, rounds=1),
    'each-65': dict(order='r'*64 + 'f'*4 + 'r', homes=[0]*5, trace=[('each', 320, 0), ('each', 5, 1)], peak=320, rounds=1),
    'each-rounds': dict(order='r'*300 + 'f'*4, homes=[0]*5, trace=[('each', 320, 0)] + [('each', 320, 1)]*3 + [('each', 220, 1)], peak=320, rounds=2),
    # ... one and four agents: the boxes in scalar registers
    # (every window a full 64 rows, the frame's four again and again: a shorter last window would take the other branch)
    'few-1': dict(order='r'*64 + 'r'*64 + 'r'*10 + 'f'*54, homes=[0], trace=[('few', 64, 0), ('few', 128, 0), ('few', 10, 1)], peak=128, rounds=1),
    'few-4-at': dict(order='r'*16 + 's'*16 + 'f'*32 + 'r'*8 + 'f'*56, homes=[0, 0, 0, 1], trace=[('few', 64, 0), ('few', 88, 0)], peak=88, rounds=1),
    'few-4-above': dict(order='r'*16 + 's'*17 + 'f'*31 + 'r'*8 + 'f'*56, homes=[0, 0, 0, 1], trace=[('few', 65, 0), ('few', 24, 1)], peak=65, rounds=1),
    # an odd row in a window sends it down the other branch, for the four agents too - and so does a last window of fewer than 64 rows
    'few-odd': dict(order='r'*30 + 'n' + 't' + 'f'*32 + 'r'*8 + 'f'*56 + 'r'*8 + 'f'*4, homes=[0, 0, 0, 0],
                    trace=[('each', 128, 0), ('few', 32, 1), ('each', 64, 0)], peak=128, rounds=1),
}


def sweep(name):
    """(rosette, spec) of a SWEEPS entry."""
    spec = SWEEPS[name]
    return Rosette(spec['order'], spec['homes']), spec


def check_sweep(name, heading=0.):
    """A SWEEPS entry's counted facts at one heading: every (row, agent) pair's margins, the sweep's trace, peak and rounds."""
    ros, spec = sweep(name)
    tasks = ros.tasks(heading)
    touch, odd = boxes_touch(tasks, ros.rows), odd_rows(ros.rows)
    near = in_reach(tasks, ros.rows)
    ring = np.array([k in 'rnt' for k in ros.order]), np.array([k == 's' for k in ros.order])
    for t, home in enumerate(ros.homes):                                 # (in reach and touching: the agent's own ring, nothing else)
        assert np.array_equal(touch[t], ring[home]) and np.array_equal(near[t], ring[home] | odd), (name, t)
    trace, peak = sweep_trace(touch, odd)
    assert trace == spec['trace'] and peak == spec['peak'] and rounds(len(ros.rows)) == spec['rounds'], (name, trace, peak)
    return ros


# the gridded worlds: ring walls first, the frame behind them; the near lists are read from the grid on the device's side
GRIDDED = {
    'deal-64': dict(order='r'*64 + 'f'*4, homes=[0], P=64, kept=None),                      # one pair a lane, cull and test
    'deal-65': dict(order='r'*65 + 'f'*4, homes=[0], P=65, kept=[64, 1]),                   # the cull first, compacted
    'deal-full': dict(order='r'*5 + 'f'*4, homes=[0]*64, P=320, kept=[64]*5),               # the list fills to its last slot, no flush
    'deal-flush': dict(order='r'*6 + 'f'*4, homes=[0]*64, P=384, kept=[64]*6),              # ... and one window more: a flush mid-deal
}


def gridded(name):
    spec = GRIDDED[name]
    return Rosette(spec['order'], spec['homes']), spec


def check_gridded(name, counts=None, lists=None, heading=0.):
    """A GRIDDED entry's counted facts: the margins, and - the near lists given (`counts` rows an agent, `lists` the rows) - P, the
    pairs kept window by window and what the list makes of them. Without the lists: what they must be for the counts to come out
    (every ring wall, nothing of the frame)."""
    ros, spec = gridded(name)
    tasks = ros.tasks(heading)
    ring = np.array([k == 'r' for k in ros.order])
    assert all(np.array_equal(v, ring) for v in in_reach(tasks, ros.rows))
    if counts is None:
        counts, lists = [int(ring.sum())]*len(tasks), [ros.rows[ring]]*len(tasks)
    P, kept = deal_windows(counts, [[not beyond(task, row) for row in rows] for task, rows in zip(tasks, lists)])
    assert P == spec['P'], (name, P)
    if spec['kept'] is not None:
        assert P > WAVE and kept == spec['kept'], (name, kept)
        lengths, flushes, peak = list_trace(kept, PHYS_PAIRS)
        assert peak == min(P, PHYS_PAIRS) and flushes == (P > PHYS_PAIRS), (name, lengths)
    else:
        assert P <= WAVE
    return ros


# rollout_walls_kernel: one agent, K candidates that all start where it stands and take row 1 of straight() at step 0
# (`swept`: the list's length behind every window without a grid - a candidate's rows are the env's, the frame's four in the last
# window; `listed`: with one - its rows are its cell's near list, the ring)
ROLLED = {
    'walls-64': dict(order='r'*64, K=5, swept=[64, 64, 128, 128, 192, 192, 256, 0, 64, 64], listed=[64, 128, 192, 256, 64], flushes=1, peak=256),
    'walls-65': dict(order='r'*65, K=5, swept=[64, 65, 129, 130, 194, 1, 65, 66, 130, 131], listed=[64, 65, 129, 130, 194, 1, 65, 66, 130, 131],
                     flushes=1, peak=194),
    # 193 = ROLL_PAIRS - 63: the shortest list that is flushed before a window is appended
    'walls-129': dict(order='r'*129, K=3, swept=[64, 128, 129, 193, 64, 65, 129, 193, 1], listed=[64, 128, 129, 193, 64, 65, 129, 193, 1],
                      flushes=2, peak=193),
    # one candidate alone overflows the list and flushes inside its own rows
    'walls-300': dict(order='r'*300, K=2, swept=[64, 128, 192, 256, 44, 108, 172, 236, 64, 108], listed=[64, 128, 192, 256, 44, 108, 172, 236, 64, 108],
                      flushes=2, peak=256),
}


def straight(T=7):
    """A table that never turns: table(T) without its turns - at heading 0 its deltas are the velocities, on any libm. (Of seven
    rows: row 4 goes straight through the rosette's gap.)"""
    t = table(T, turning=False)
    if T == 7:
        t[4] = (-3.5, 0., 0.)
    return t


def rolled(name):
    spec = ROLLED[name]
    return Rosette(spec['order'] + 'f'*4, [0]), spec


def check_rolled(name, lists=None):
    """A ROLLED entry at step 0 (keep = 0, heading 0: a candidate's velocity is its action's row): margins, and the list's lengths
    window by window - over the env's rows, or (`lists`: the rows of each candidate's near list) over those."""
    ros, spec = rolled(name)
    plans = rolled_plans(name)
    tab = straight()
    tasks = [task_of(ros.positions[0], tab[plans[k, 0]][:2]) for k in range(spec['K'])]
    near = in_reach(tasks, ros.rows)
    ring = np.array([k == 'r' for k in ros.order])
    assert all(np.array_equal(v, ring) for v in near)
    if lists is not None:
        assert all(len(rows) == int(ring.sum()) for rows in lists)
        near = [[not beyond(task, row) for row in rows] for task, rows in zip(tasks, lists)]
    lengths, flushes, peak = list_trace(rollout_windows(near), ROLL_PAIRS)
    assert (lengths, flushes, peak) == (spec['swept' if lists is None else 'listed'], spec['flushes'], spec['peak']), (name, lengths, flushes, peak)
    return ros


def rolled_plans(name, H=3):
    """(K, H) plans over straight(): every candidate moves (rows 1 .. 6), so every ring wall is in its reach at step 0."""
    K = ROLLED[name]['K']
    plans = (1 + (np.arange(K)[:, None]*2 + np.arange(H)[None]*3) % 6).astype(np.int64)
    plans[-1] = 4                                                        # (the last candidate leaves through the gap and meets nothing)
    return plans


# walk_rows: spots whose cells' near lists hold 0, 1, 3, 4 and 5 rows (ROLL_AHEAD = 4), and one spot outside the grid
SPOTS = np.array([[4., 4.], [9., 4.], [14., 4.], [19., 4.], [24., 4.], [-30., 4.]])
SPOT_ROWS = (0, 1, 3, 4, 5, None)                                        # (None: no list covers it - it walks every row)


def spots_world():
    """(rows, positions): a 28 m x 8 m frame and, round spot i, SPOT_ROWS[i] short walls 25 cm from it."""
    rows = [[0, 0, 28, 0], [28, 0, 28, 8], [28, 8, 0, 8], [0, 8, 0, 0]]
    for (x, y), n in zip(SPOTS, SPOT_ROWS):
        for j in range(n or 0):
            a = 2*np.pi*(j + .25)/n
            mid, tangent = np.array([x + .25*np.cos(a), y + .25*np.sin(a)]), np.array([-np.sin(a), np.cos(a)])
            rows.append(np.concatenate([mid - .03*tangent, mid + .03*tangent]))
    return np.asarray(rows, F), SPOTS.astype(F)


# the rosettes' launches: everybody along each in turn (100 and 240: where the rings of five and six walls make somebody slide)
HEADINGS = (0., 45., 90., 100., 135., 180., 225., 240., 270., 315.)


def spots_check():
    """Round spot i exactly SPOT_ROWS[i] rows nearer than 30 cm - well inside the near lists' short tier - and every other row
    farther than 3 m - well outside their long one."""
    rows, spots = spots_world()
    for spot, n in zip(spots[:-1], SPOT_ROWS[:-1]):
        d = np.array([distance(spot, row) for row in rows])
        assert (d < .3).sum() == n and ((d < .3) | (d > 3.)).all()
    assert min(distance(spots[-1], row) for row in rows) > 3. and spots[-1][0] < 0
    return rows, spots
