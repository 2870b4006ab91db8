"""The DEVICE builds of the culls and shortcuts, element by element (include/megastep_hip_test.h, ms_test_*; kernels/culltest.h),
where the device does not compile the host's text: v_rcp_f32 for a division in wall_beyond, ray_interval, pseudo_angle_fast and
wg_cell_at, one refined reciprocal for tex_filter's two divisions, sign tests for light_blocked's two quotients - and agents_apart,
whose text is the same.  Each is held to the oracle (or to the plain rule the suite already states) on the operands of the CPU
tests of the host instantiations (tests/cull_samples.py) and at its thresholds.  Where the issue of a comparison with the host
instantiation is a figure, not a condition, it is printed (pytest -s): DESIGN.md section 2 records what an MI355X gave."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import cull_samples, shade_rule, util

pytestmark = pytest.mark.gpu

F = np.float32
F32P, I32P = C.POINTER(C.c_float), C.POINTER(C.c_int)


def _device(name, ins, outs, scalars=()):
    """ms_test_<name>(*ins, *scalars, *outs, count, stream) on device copies of `ins`: the outputs (dtypes `outs`) as numpy."""
    from megastep_amd import _lib
    dev = torch.device('cuda')
    tin = [torch.as_tensor(np.ascontiguousarray(a), device=dev) for a in ins]
    count = len(ins[0])
    tout = [torch.empty(count, dtype=dt, device=dev) for dt in outs]
    ptr = lambda t: C.c_void_p(t.data_ptr())
    _lib.check(getattr(_lib.lib(), 'ms_test_' + name)(*map(ptr, tin), *scalars, *map(ptr, tout), count,
                                                      C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in tout]


def _rows(a):
    """A pointer to each row of four floats of a contiguous (n, 4) float32 array."""
    assert a.dtype == np.float32 and a.flags.c_contiguous and a.shape[1] == 4
    return [C.cast(a.ctypes.data + 16*i, F32P) for i in range(len(a))]


def _nudged(x, ulps):
    """binary32 x moved by `ulps` (ints: up for positive, down for negative) steps through the floats."""
    x, ulps = np.array(x, F), np.broadcast_to(np.asarray(ulps), np.shape(x))
    towards = np.where(ulps > 0, F(np.inf), F(-np.inf)).astype(F)
    for step in range(1, int(np.abs(ulps).max(initial=0)) + 1):
        x = np.where(np.abs(ulps) >= step, np.nextafter(x, towards), x).astype(F)
    return x


# ---- agents apart ------------------------------------------------------------------------------------------------------

def test_agents_the_device_calls_apart_cannot_collide(oracle):
    """The CPU test's pairs through the device build of agents_apart: every pair it calls apart leaves the oracle's collision_cc at
    1, every collision is kept, the cull culls - and, the text being the same, contraction off and the divisions correctly rounded on
    both sides, its bytes are ms_host_agents_apart's on every pair."""
    from megastep_amd import _lib
    me, other, R = cull_samples.agent_pairs()
    n = len(me)
    assert n == 60000
    apart = _device('agents_apart', [me, other, R], [torch.uint8])[0].astype(bool)
    cc, radii = oracle.lib().oracle_collision_cc, R.tolist()
    x = np.array([cc(*me[i].tolist(), *other[i].tolist(), radii[i]) for i in range(n)], F)
    bad = apart & ~(x == 1)
    assert not bad.any(), (np.flatnonzero(bad)[:5], me[bad][:5], other[bad][:5], R[bad][:5], x[bad][:5])
    in_step = (me[:, 2:] == other[:, 2:]).all(1)                         # (in step: never collide)
    assert ((np.isfinite(me).all(1) & np.isfinite(other).all(1)) | in_step)[apart].all()
    hits, hits_kept, culled = int((x < 1).sum()), int(((x < 1) & ~apart).sum()), int(apart.sum())
    assert hits > n//20 and hits_kept == hits, 'the sample holds plenty of collisions, none of them culled'
    assert culled > n//4, 'and the cull does cull'
    host = _lib.lib().ms_host_agents_apart
    on_host = np.array([host(a, b, r) for a, b, r in zip(_rows(me), _rows(other), radii)], bool)
    differ = on_host != apart
    print(f'agents_apart: {int(differ.sum())} of {n} device verdicts differ from the host\'s')
    assert not differ.any(), (np.flatnonzero(differ)[:5], me[differ][:5], other[differ][:5], R[differ][:5])


# ---- walls beyond reach ------------------------------------------------------------------------------------------------

def _cs_of(oracle, agents, walls, radii):
    cs = oracle.lib().oracle_collision_cs
    return np.array([cs(*agents[i].tolist(), *walls[i].tolist(), radii[i]) for i in range(len(agents))], F)


def _host_beyond(agents, walls, radii):
    from megastep_amd import _lib
    host = _lib.lib().ms_host_wall_beyond_reach
    return np.array([host(a, w, r) for a, w, r in zip(_rows(agents), _rows(walls), radii)], bool)


def test_walls_the_device_calls_beyond_reach_cannot_stop_the_agent(oracle):
    """The CPU test's agents and walls through the device builds of wall_reach, reach_squared and wall_beyond (the foot of the
    perpendicular through v_rcp_f32, where the host divides): every wall called beyond leaves the oracle's collision_cs at 1, every
    collision is kept, the cull culls.  Then at the threshold itself: for 4000 of the pairs the wall is slid along the line from the
    agent through its middle, the HOST's verdict bisected down to two adjacent binary32 distances, and the device asked about the nine
    distances round them - the same property on every one.  How often the two builds disagree there is printed, not asserted."""
    from megastep_amd import _lib
    agents, walls, R = cull_samples.agents_and_walls()
    n, radii = len(agents), R.tolist()
    assert n == 80000
    reach, beyond = _device('wall_beyond', [agents, walls, R], [torch.float32, torch.uint8])
    beyond = beyond.astype(bool)
    x = _cs_of(oracle, agents, walls, radii)
    bad = beyond & ~(x == 1)
    assert not bad.any(), (np.flatnonzero(bad)[:5], agents[bad][:5], walls[bad][:5], R[bad][:5], x[bad][:5])
    assert (np.isfinite(agents[:, :2]).all(1) & np.isfinite(walls).all(1))[beyond].all()     # (a NaN is never beyond)
    hits, hits_kept, culled = int((x < 1).sum()), int(((x < 1) & ~beyond).sum()), int(beyond.sum())
    assert hits > n//20 and hits_kept == hits, 'the sample holds plenty of collisions, none of them culled'
    assert culled > n//4, 'and the cull does cull'
    # the reach is the same text on both sides (a correctly rounded division and square root): the same bits
    host_reach = _lib.lib().ms_host_wall_reach
    want = np.array([host_reach(a, r) for a, r in zip(_rows(agents), radii)], F)
    same = (want.view(np.uint32) == reach.view(np.uint32)) | (np.isnan(want) & np.isnan(reach))
    assert same.all(), (np.flatnonzero(~same)[:5], agents[~same][:5], reach[~same][:5], want[~same][:5])
    on_host = _host_beyond(agents, walls, radii)
    print(f'wall_beyond, the CPU test\'s pairs: {int((on_host != beyond).sum())} of {n} device verdicts differ from the host\'s')

    # the threshold: wall k with its middle d metres from the agent, along the line it was on
    finite = np.isfinite(agents).all(1) & np.isfinite(walls).all(1)
    p, mid = agents[:, :2].astype(np.float64), .5*(walls[:, :2].astype(np.float64) + walls[:, 2:])
    away = mid - p
    norm = np.linalg.norm(away, axis=1)
    finite &= norm > 0

    def slid(sel, d):
        u = away[sel]/norm[sel, None]
        shift = p[sel] + d.astype(np.float64)[:, None]*u - mid[sel]
        return np.ascontiguousarray(walls[sel].astype(np.float64) + np.tile(shift, 2), F)

    # ... bracketed by 0 (the wall across the agent) and four reaches and a metre; walls too short for the cull ever to call them
    # beyond (or shorter than a float's step that far out: a crawl's reach is astronomical) have no threshold
    far = (F(4)*want + F(1)).astype(F)
    cand = np.flatnonzero(finite & np.isfinite(far))[:8000]
    rc = [radii[i] for i in cand]
    ok = ~_host_beyond(agents[cand], slid(cand, np.zeros(len(cand), F)), rc) & _host_beyond(agents[cand], slid(cand, far[cand]), rc)
    sel = cand[ok][:4000]
    assert len(sel) == 4000
    rs, ag = [radii[i] for i in sel], np.ascontiguousarray(agents[sel])
    lo, hi = np.zeros(4000, np.int64), far[sel].view(np.int32).astype(np.int64)               # (positive floats order as their bits)
    while (hi - lo > 1).any():
        m = np.where(hi - lo > 1, (lo + hi)//2, hi)
        b = _host_beyond(ag, slid(sel, m.astype(np.int32).view(F)), rs)
        lo, hi = np.where(b | (hi - lo <= 1), lo, m), np.where(b & (hi - lo > 1), m, hi)
    steps = np.arange(-4, 5)
    d9 = (hi[:, None] + steps[None]).astype(np.int32).view(F)            # hi - 4 .. hi + 4 ulps: lo = hi - 1 among them
    assert (d9 >= 0).all()
    sel9 = np.repeat(sel, 9)
    a9, w9, r9 = np.ascontiguousarray(agents[sel9]), slid(sel9, d9.ravel()), R[sel9]
    _, beyond9 = _device('wall_beyond', [a9, w9, r9], [torch.float32, torch.uint8])
    beyond9 = beyond9.astype(bool)
    x9 = _cs_of(oracle, a9, w9, r9.tolist())
    bad = beyond9 & ~(x9 == 1)
    assert not bad.any(), (int(bad.sum()), a9[bad][:5], w9[bad][:5], r9[bad][:5], x9[bad][:5])
    # (the host's verdict flips between hi - 1 and hi: four of the nine distances on the near side, five on the far side)
    assert beyond9.sum() > len(beyond9)//4 and (~beyond9).sum() > len(beyond9)//4, 'the nine distances straddle the device\'s threshold too'
    host9 = _host_beyond(a9, w9, r9.tolist())
    print(f'wall_beyond, nine distances round the host\'s threshold: {int((host9 != beyond9).sum())} of {len(beyond9)} device verdicts '
          f'differ from the host\'s ({int((beyond9 & ~host9).sum())} beyond on the device only)')


# ---- ray intervals -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('res,fov', cull_samples.RAY_SHAPES)
def test_no_ray_outside_a_lines_device_interval_hits_it(oracle, res, fov):
    """The CPU test's lines through the device build of agent_frame + ray_interval (y/x through v_rcp_f32), waves of one group and of
    the shape's NG: every ray the oracle's render lands on the line lies inside the device's interval, the intervals lie inside the
    wave, and they are no wider than the CPU test allows the host's."""
    from megastep_amd import _lib
    lib = _lib.lib()
    poses, lines, idx, M, radius = cull_samples.lines_in_view(oracle, res, fov)
    E = len(poses)
    assert E == 3000
    hits = covered = differ = total = worst = 0
    pose_rows, line_rows = _rows(poses), _rows(lines)
    for groups in sorted({1, cull_samples.groups_for(res)}):
        W = 64*groups
        for g in range((res + W - 1)//W):
            first, rays = _device('ray_interval', [poses, lines], [torch.int32, torch.int32], (res, fov, radius, groups, g))
            room = min(W, res - W*g)
            inside = (rays == 0) | ((first >= 0) & (rays > 0) & (first + rays <= room))
            assert inside.all(), (groups, g, first[~inside][:5], rays[~inside][:5])
            on = idx[:, W*g:W*g + W] == M
            leftmost, rightmost = on.argmax(1), on.shape[1] - 1 - on[:, ::-1].argmax(1)
            held = ~on.any(1) | ((leftmost >= first) & (rightmost < first + rays))
            assert held.all(), (groups, g, np.flatnonzero(~held)[:5], first[~held][:5], rays[~held][:5], poses[~held][:5], lines[~held][:5])
            if groups == 1:
                hits += int(on.sum())
                covered += int(rays.sum())
            lo, cnt = C.c_int(), C.c_int()
            for e, (pose, line) in enumerate(zip(pose_rows, line_rows)):
                lib.ms_host_ray_interval_wide(pose, line, res, fov, radius, groups, g, C.byref(lo), C.byref(cnt))
                a, b, c, d = int(first[e]), int(first[e] + rays[e]), lo.value, lo.value + cnt.value
                apart = (b - a) + (d - c) - 2*max(0, min(b, d) - max(a, c))       # rays in one interval and not in the other
                differ += apart > 0
                worst = max(worst, apart)
            total += E
    assert hits > E*res//200, 'plenty of rays land on their wall'
    assert covered < 8*hits + E, 'and the intervals are not much wider than what they must hold'
    print(f'ray_interval {res} rays, fov {fov:g}: {differ} of {total} device intervals differ from the host\'s, by {worst} rays at most')


# ---- the wedge ---------------------------------------------------------------------------------------------------------

def test_a_waves_device_wedge_holds_every_ray_of_its_fan(oracle):
    """pseudo_angle_fast + wg_wedge as render_kernel forms a wave's run of directions - from its rightmost ray to its leftmost - for
    the fans of the six shapes at 4096 random headings, waves of one group and of the shape's NG: the run [wa8, wb8] holds the step
    floor(64 p) of the binary64 pseudo-angle p of every ray of the wave.  (WG_ARC_MARGIN is 0.128 of a step, the hardware
    reciprocal's error 1e-5 of one: the binary64 value is inside with room to spare.)  A NaN direction gives the full run."""
    from megastep_amd import _lib
    lib = _lib.lib()
    differ = total = 0
    for res, fov in cull_samples.RAY_SHAPES:
        rng = np.random.RandomState(res)
        H = 4096
        sn, cs = oracle.sincospi_many(rng.uniform(-180, 180, H).astype(F)/F(180))
        half_screen = F(np.tan(np.pi/180*fov/2))
        r = np.arange(res, dtype=F)
        uy = (F(res) - F(2)*r - F(1))*half_screen/F(res)                    # ray_y, kernels.cu:234-236, in binary32 as the kernel
        rays = np.stack([cs[:, None] - sn[:, None]*uy[None], sn[:, None] + cs[:, None]*uy[None]], -1).astype(F)   # (H, res, 2)
        x, y = rays[..., 0].astype(np.float64), rays[..., 1].astype(np.float64)
        p = y/(np.abs(x) + np.abs(y))
        p = np.where(x < 0, 2 - p, np.where(p < 0, 4 + p, p))
        step = np.floor(64*p).astype(np.int64) & 255
        for groups in sorted({1, cull_samples.groups_for(res)}):
            W = 64*groups
            for g in range((res + W - 1)//W):
                first, last = W*g, min(W*g + W - 1, res - 1)               # rays run from the left of the view to its right
                right, left = np.ascontiguousarray(rays[:, last]), np.ascontiguousarray(rays[:, first])
                wa, wb = _device('wedge', [right, left], [torch.int32, torch.int32])
                assert ((wa >= 0) & (wa < 256) & (wb >= 0) & (wb < 256)).all()
                held = ((step[:, first:last + 1] - wa[:, None]) & 255) <= ((wb - wa) & 255)[:, None]
                assert held.all(), (res, fov, groups, g, np.argwhere(~held)[:5])
                assert groups > 1 or res < 64 or (((wb - wa) & 255) < 200).all(), 'a fan below 180 degrees is no full run'
                a8, b8 = C.c_int(), C.c_int()
                for h in range(H):
                    lib.ms_host_wedge(*right[h].tolist(), *left[h].tolist(), C.byref(a8), C.byref(b8))
                    differ += (a8.value, b8.value) != (int(wa[h]), int(wb[h]))
                total += H
    nan = float('nan')
    right = np.array([[nan, 1], [1, nan], [1, 0], [1, 0], [nan, nan]], F)
    left = np.array([[0, 1], [0, 1], [nan, 1], [0, nan], [nan, nan]], F)
    wa, wb = _device('wedge', [right, left], [torch.int32, torch.int32])
    assert (wa == 0).all() and (wb == 255).all()
    print(f'wedge: {differ} of {total} device runs differ from the host\'s wg_wedge(pseudo_angle(..))')


# ---- wg_cell_at --------------------------------------------------------------------------------------------------------

def _cell_widths():
    from megastep_amd import cuda
    fine = cuda.Scenery.WALL_GRID_CELL
    built = {fine*k for k in (1, 2, 4)}                                     # grids.build_wall_grid: doubled twice at most
    built |= {w*cuda.Scenery.WALL_GRID_COARSE for w in built}              # ... each with a parent level
    return sorted(built | {cuda.Scenery.LIGHT_GRID_CELL, .3, 1/3, .7, .1})


def test_the_cell_the_device_picks_holds_the_point():
    """wg_cell_at - device text only: floor((x - x0) v_rcp_f32(cell)) - on grids of every cell width the project builds and a few
    awkward ones, origins up to a kilometre out, up to 256 cells a side; points on every cell boundary and 1, 2, 4 ulps either side
    of it, on the grid's outer edges, all over the inside, up to 2 cm outside, NaNs and infinities.  What the eight call sites lean
    on: a point called inside lies in the GROWN box (WG_SLACK, a centimetre, on every side: kernels/wallgrid.h, wg_cell_of - formed
    here in binary32 exactly as there) of the cell picked, whose lists therefore serve it; NaNs, infinities and points more than
    WG_SLACK outside the grid are outside, with index 0.  (The quotient is three roundings of a value no larger than the extent -
    under 1e-3 m at the kilometre of the widest grid here - so the binary64 conditions hold with a centimetre by an order and more,
    and a point a centimetre and more INSIDE the grid is always called inside.)"""
    rng = np.random.RandomState(5)
    slack = F(.01)
    geoms, cells, points = [], [], []
    for width in _cell_widths():
        for k in range(10):
            nx, ny = [(256, 256), (1, 1), (256, 1), (1, 256)][k] if k < 4 else rng.randint(1, 257, 2)
            origin = np.floor(rng.uniform(-1000, 1000, 2)) - .5 if k % 2 else rng.uniform(-1000, 1000, 2)     # (grids.py: floor(lo) - .5)
            gx, gy, cell = F(origin[0]), F(origin[1]), F(width)
            ex, ey = np.float64(cell)*nx, np.float64(cell)*ny
            pts = []
            for axis, (g0, n_, e_, go, eo) in enumerate([(gx, nx, ex, gy, ey), (gy, ny, ey, gx, ex)]):
                # every k x cell boundary as the builder forms it, the outer edges among them, and 1, 2, 4 ulps either side
                edge = (g0 + np.arange(n_ + 1, dtype=F)*cell).astype(F)
                at = _nudged(np.repeat(edge, 7), np.tile([0, 1, -1, 2, -2, 4, -4], n_ + 1))
                other = (go + rng.uniform(0, eo, len(at))).astype(F)
                # ... and up to 2 cm outside either outer edge, the other coordinate anywhere from 2 cm outside to 2 cm outside
                out = np.where(rng.rand(400) < .5, g0 - rng.uniform(0, .02, 400), np.float64(g0) + e_ + rng.uniform(0, .02, 400)).astype(F)
                other = np.concatenate([other, (go + rng.uniform(-.02, eo + .02, 400)).astype(F)])
                at = np.concatenate([at, out])
                pts.append(np.stack([at, other] if axis == 0 else [other, at], 1))
            pts.append(np.stack([gx + rng.uniform(0, ex, 2000), gy + rng.uniform(0, ey, 2000)], 1).astype(F))
            odd = np.stack([gx + rng.uniform(0, ex, 12), gy + rng.uniform(0, ey, 12)], 1).astype(F)
            odd[np.arange(12), np.arange(12) % 2] = np.repeat(F([np.nan, np.inf, -np.inf]), 4)
            odd[-1] = np.nan
            pts.append(odd)
            pts = np.concatenate(pts)
            points.append(pts)
            geoms.append(np.tile(F([gx, gy, nx, ny]), (len(pts), 1)))
            cells.append(np.full(len(pts), cell, F))
    geom, cell, pt = np.concatenate(geoms), np.concatenate(cells), np.concatenate(points)
    index, inside = _device('cell_at', [geom, cell, pt], [torch.int32, torch.uint8])
    inside = inside.astype(bool)
    nx, ny = geom[:, 2].astype(np.int64), geom[:, 3].astype(np.int64)
    finite = np.isfinite(pt).all(1)
    assert (~finite).sum() >= 12 and not inside[~finite].any()
    assert (index[~inside] == 0).all()
    assert ((index >= 0) & (index < nx*ny)).all()
    ix, iy = index % nx, index//nx
    with np.errstate(invalid='ignore'):
        rel = pt.astype(np.float64) - geom[:, :2]
        extent = cell.astype(np.float64)[:, None]*np.stack([nx, ny], 1)
        beyond = ((rel < -np.float64(slack)) | (rel > extent + np.float64(slack))).any(1)
        within = ((rel >= np.float64(slack)) & (rel <= extent - np.float64(slack))).all(1)
    assert beyond.sum() > 1000 and not inside[beyond].any()
    assert within.sum() > 100000 and inside[within].all()
    for axis, i in ((0, ix), (1, iy)):
        # k.x0 = geom.x + ix*cell - WG_SLACK; k.x1 = k.x0 + cell + 2*WG_SLACK, every operation rounded to binary32
        x0 = ((geom[:, axis] + i.astype(F)*cell).astype(F) - slack).astype(F)
        x1 = ((x0 + cell).astype(F) + F(2)*slack).astype(F)
        held = ~inside | ((pt[:, axis] >= x0) & (pt[:, axis] <= x1))
        assert held.all(), (axis, geom[~held][:5], cell[~held][:5], pt[~held][:5], index[~held][:5])
    with np.errstate(invalid='ignore'):
        exact = np.floor(rel/cell.astype(np.float64)[:, None])
    other_cell = inside & ((exact[:, 0] != ix) | (exact[:, 1] != iy))
    print(f'wg_cell_at: {int(other_cell.sum())} of {int(inside.sum())} points called inside ({other_cell.sum()/inside.sum():.2%}) are in another '
          f'cell than the binary64 floor\'s; {len(pt)} points in all')


# ---- tex_filter --------------------------------------------------------------------------------------------------------

def test_the_devices_texel_filter_is_the_references():
    """tex_filter (one refined reciprocal for both weights) against tests/shade_rule.py's, the reference's filter with its two true
    divisions: the two texels and the BITS of the two weights, for rows of 1 .. 64 texels and of 1000 - at 0, at 1, at every
    k/(w + 1), where a texel's share passes through its extremes, and 2 ulps either side of it, and at 100 000 places drawn uniformly."""
    rng = np.random.RandomState(6)
    xs, ws = [], []
    for w in list(range(1, 65)) + [1000]:
        at = (np.arange(w + 2, dtype=F)/F(w + 1)).astype(F)
        near = np.concatenate([at[1:], _nudged(at[1:], 1), _nudged(at[1:], 2), _nudged(at[1:], -1), _nudged(at[1:], -2)])    # (0 has no float 2 ulps below it)
        x = np.concatenate([F([0, 1, 1e-45, 3e-45]), near])
        xs.append(x)
        ws.append(np.full(len(x), w, np.int32))
    m = 100_000
    xs.append(rng.uniform(0, 1, m).astype(F))
    ws.append(rng.choice(list(range(1, 65)) + [1000], m).astype(np.int32))
    x, w = np.concatenate(xs), np.concatenate(ws)
    l, r, lw, rw = _device('tex_filter', [x, w], [torch.int32, torch.int32, torch.float32, torch.float32])
    want = [shade_rule.tex_filter(xi, wi) for xi, wi in zip(x, w.tolist())]
    wl, wr = np.array([t[0] for t in want], np.int32), np.array([t[1] for t in want], np.int32)
    wlw, wrw = np.array([t[2] for t in want], F), np.array([t[3] for t in want], F)
    bad = (l != wl) | (r != wr) | (lw.view(np.uint32) != wlw.view(np.uint32)) | (rw.view(np.uint32) != wrw.view(np.uint32))
    assert not bad.any(), (int(bad.sum()), x[bad][:5], w[bad][:5], l[bad][:5], wl[bad][:5], r[bad][:5], wr[bad][:5], lw[bad][:5], wlw[bad][:5],
                           rw[bad][:5], wrw[bad][:5])


# ---- light_blocked -----------------------------------------------------------------------------------------------------

def _signed(rng, lo, hi, shape):
    """Magnitudes log-uniform in [lo, hi], either sign."""
    return (np.exp(rng.uniform(np.log(lo), np.log(hi), shape))*rng.choice([-1., 1.], shape)).astype(F)


def _blocked_both_ways(I, U, a, v):
    got = _device('light_blocked', [I, U, a, v], [torch.uint8])[0].astype(bool)
    return got, util.obstructed_pairs(I, U, a, v)


def test_the_devices_shadow_test_is_the_references_obstructed():
    """light_blocked - `obstructed` (kernels.cu:253-257) without its two divisions: sign tests on the numerators for 0 < t < 1 and
    0 < s, one division for s < .999 - against the plain binary32 statement the suite already has (tests/util.py), byte for byte: a
    million pairs of a light, a point and a wall with coordinates of magnitude 2^-10 .. 2^10, and the awkward ones - |UxV| within 2 ulps
    of 1e-3, the numerator of t within 2 ulps of |UxV|, s within 2 ulps of .999, zero numerators of either sign, a NaN or an infinity
    in each slot."""
    rng = np.random.RandomState(7)
    m = 1_000_000
    I, U, a, v = (_signed(rng, 2.**-10, 2.**10, (m, 2)) for _ in range(4))
    k = 200_000                                                            # walls near their light, so that a fifth of the pairs can block at all
    a[:k] = (I[:k] + U[:k]*rng.uniform(0, 1.2, (k, 1)).astype(F) - v[:k]*rng.uniform(-.2, 1.2, (k, 1)).astype(F)).astype(F)

    # The awkward ones, on axes so that every product is one rounding: U = (ux, 0), V = (0, vy), I = 0 - UxV = ux vy, t's numerator
    # -a.y ux, s = a.x vy/(ux vy) - and the same turned a quarter (U = (0, uy), V = (vx, 0): UxV of the other sign)
    def on_axes(ux, vy, ax, ay, turned):
        n = len(ux)
        z = np.zeros(n, F)
        Ux, Vx, Ax = np.stack([ux, z], 1), np.stack([z, vy], 1), np.stack([ax, ay], 1)
        t = np.asarray(turned, bool)[:, None]
        return (np.zeros((n, 2), F), np.where(t, Ux[:, ::-1], Ux).astype(F), np.where(t, Ax[:, ::-1], Ax).astype(F),
                np.where(t, Vx[:, ::-1], Vx).astype(F))

    q = 20_000
    sets = []
    # |UxV| = 1e-3 and 1, 2, 3 ulps either side of it, exactly: vy a power of two
    vy = (2.**rng.randint(-8, 9, q)).astype(F)*rng.choice(F([-1, 1]), q)
    ux = (_nudged(np.full(q, 1e-3, F), rng.randint(-3, 4, q))/np.abs(vy)).astype(F)*rng.choice(F([-1, 1]), q)
    assert set((np.abs(ux*vy).view(np.int32) - F(1e-3).view(np.int32)).tolist()) == set(range(-3, 4))
    s, t = rng.uniform(.05, .95, q), rng.uniform(.05, .95, q)
    sets.append(on_axes(ux, vy, (s*ux).astype(F), (-t*vy).astype(F), rng.rand(q) < .5))
    # t's numerator 0 .. 3 ulps either side of |UxV|: a.y = -vy moved by ulps
    ux, vy = _signed(rng, .05, 30, q), _signed(rng, .05, 30, q)
    ay = _nudged(-vy, rng.randint(-3, 4, q))
    sets.append(on_axes(ux, vy, (rng.uniform(.05, .95, q)*ux).astype(F), ay, rng.rand(q) < .5))
    # s 0 .. 4 ulps either side of .999
    ux, vy = _signed(rng, .05, 30, q), _signed(rng, .05, 30, q)
    ax = _nudged((F(.999)*ux).astype(F), rng.randint(-4, 5, q))
    with np.errstate(all='ignore'):
        s_bits = ((ax*vy)/(ux*vy)).astype(F).view(np.int32) - F(.999).view(np.int32)
    assert set(range(-2, 3)) <= set(s_bits.tolist())
    sets.append(on_axes(ux, vy, ax, (-rng.uniform(.05, .95, q)*vy).astype(F), rng.rand(q) < .5))
    # zero numerators of either sign: a.x = +-0 (s), a.y = +-0 (t), the wall's end on the light
    ux, vy = _signed(rng, .05, 30, q), _signed(rng, .05, 30, q)
    ax = np.where(rng.rand(q) < .5, rng.choice(F([0., -0.]), q), (rng.uniform(.05, .95, q)*ux).astype(F)).astype(F)
    ay = np.where(rng.rand(q) < .5, rng.choice(F([0., -0.]), q), (-rng.uniform(.05, .95, q)*vy).astype(F)).astype(F)
    sets.append(on_axes(ux, vy, ax, ay, rng.rand(q) < .5))
    # a NaN or an infinity in each slot of pairs that block without it
    ux, vy = _signed(rng, .05, 30, 24), _signed(rng, .05, 30, 24)
    odd = [x.copy() for x in on_axes(ux, vy, (F(.5)*ux).astype(F), (F(-.5)*vy).astype(F), np.zeros(24, bool))]
    plain = [x.copy() for x in odd]
    for j in range(24):
        odd[j//6][j, (j//3) % 2] = [np.nan, np.inf, -np.inf][j % 3]
    sets += [tuple(plain), tuple(odd)]

    I, U, a, v = (np.ascontiguousarray(np.concatenate([x] + [st[j] for st in sets])) for j, x in enumerate((I, U, a, v)))
    got, want = _blocked_both_ways(I, U, a, v)
    assert want[:m].sum() > m//100 and want[m:m + 4*q].sum() > q and want[m + 4*q:m + 4*q + 24].all(), 'the sample holds plenty of shadows'
    bad = got != want
    assert not bad.any(), (int(bad.sum()), np.flatnonzero(bad)[:5], I[bad][:5], U[bad][:5], a[bad][:5], v[bad][:5], want[bad][:5])


def test_the_devices_shadow_test_where_numerators_go_denormal():
    """The same with coordinates down to 1e-30, where the numerators go denormal and the reference's quotient can underflow to zero
    while the sign of its numerator does not: light_blocked is exact wherever a numerator that is not zero exceeds 2^-150 |UxV|
    (kernels/lighting.h), and every disagreement here must be a pair outside that range - they are counted and
    printed."""
    rng = np.random.RandomState(8)
    m = 1_000_000
    I, U, a, v = (_signed(rng, 1e-30, 2.**10, (m, 2)) for _ in range(4))
    # half of them aimed: the light at the origin, U and V of everyday size (|UxV| up to 2^21), the wall's first end within
    # 1e-45 .. 1e-36 of the light: both numerators denormals or next to one, their quotients at the bottom of the denormals
    k = m//2
    U[:k], v[:k] = _signed(rng, .5, 2.**10, (k, 2)), _signed(rng, .5, 2.**10, (k, 2))
    I[:k] = 0
    a[:k] = _signed(rng, 1e-45, 1e-36, (k, 2))
    got, want = _blocked_both_ways(I, U, a, v)
    bad = got != want
    with np.errstate(all='ignore'):
        d = np.abs((U[:, 0]*v[:, 1] - U[:, 1]*v[:, 0]).astype(np.float64))             # (in binary32, as both sides form them)
        PQ = a - I
        ns = np.abs((PQ[:, 0]*v[:, 1] - PQ[:, 1]*v[:, 0]).astype(np.float64))
        nt = np.abs((PQ[:, 0]*U[:, 1] - PQ[:, 1]*U[:, 0]).astype(np.float64))
    in_range = ((ns == 0) | (ns > 2.**-150*d)) & ((nt == 0) | (nt > 2.**-150*d))
    print(f'light_blocked, coordinates down to 1e-30: {int(bad.sum())} of {m} verdicts differ from obstructed\'s '
          f'({int((bad & got).sum())} blocked on the device only); {int((~in_range).sum())} pairs have a numerator at or below 2^-150 |UxV|; '
          f'{int(want.sum())} block')
    assert not (bad & in_range).any(), (int((bad & in_range).sum()), I[bad & in_range][:5], U[bad & in_range][:5], a[bad & in_range][:5],
                                        v[bad & in_range][:5])
