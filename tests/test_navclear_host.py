"""Clearance (`ms_nav_clearance` / `ms_nav_clear_query`, `cuda.clearance_fields`, `cuda.clearance`, `modules.Proximity`) on the CPU:
the contract of include/megastep_hip.h (MsNavClearance, MsNavClearQuery) restated in binary32 numpy (`clear_rule`, which
tests/test_gpu_navclear.py holds the kernels to, bit for bit), the host instantiations of the kernels' own pieces
(ms_host_nav_clearance / ms_host_nav_clear_query: csrc/kernels/navclear.h) held to EQUALITY with it - brute force, with the tile cull
and with both culls, on floorplans and on worlds made to strain the culls - the free bytes against nav_rule's, the distances against
float64, the query against the field, the C-ABI's declarations, layouts and refusals, and the Proximity module on a stand-in."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests.test_abi import ROOT, declared_symbols
from tests.test_navfield_host import CELL, CELLS, RADIUS, _distance_to_walls, bits, nav_rule, plans
from tests.test_overhead_host import line_d2

F = np.float32
INF = F(np.inf)
NONE = np.iinfo(np.int32).max
BRUTE, TILE, TILE_WAVE = 0, 1, 2
RANGES = (.3, 2., 50.)              # the field mostly +inf, mixed, and without any


class clear_rule:
    """The contract in numpy: every operation one binary32 operation, in the order the header gives."""

    @staticmethod
    def winner(x, y, rows, R, first=0, skipped=()):
        """(d2, l, t) of the winner at points (x, y) (arrays of one shape) over `rows` (L, 4), numbered from `first`; l = NONE
        without one.  `skipped`: row numbers passed over."""
        R2 = F(R)*F(R)
        bd, bi, bt = np.full(x.shape, INF, F), np.full(x.shape, NONE, np.int64), np.zeros(x.shape, F)
        for k, line in enumerate(np.asarray(rows, F).reshape(-1, 4)):
            l = first + k
            if l in skipped:
                continue
            d2, t = line_d2(x, y, line)
            with np.errstate(invalid='ignore'):
                take = (d2 <= R2) & ((d2 < bd) | ((d2 == bd) & (l < bi)))
            bd, bi, bt = np.where(take, d2, bd).astype(F), np.where(take, l, bi), np.where(take, t, bt).astype(F)
        return bd, bi, bt

    @staticmethod
    def field(walls, geom, cell, R, radii=(), first=0):
        """(values (ny, nx) float32, nearest (ny, nx) int32, fits (K, ny, nx) uint8) of one env."""
        x, y = nav_rule.centres(geom, cell)
        x, y = np.broadcast_arrays(x[None, :], y[:, None])
        bd, bi, _ = clear_rule.winner(x, y, walls, R, first)
        won = bi != NONE
        values = np.where(won, np.sqrt(bd), INF).astype(F)
        nearest = np.where(won, bi, -1).astype(np.int32)
        fits = np.stack([np.where(won & (bd <= F(r)*F(r)), 0, 1).astype(np.uint8) for r in radii]) if len(radii) else np.zeros((0,) + x.shape, np.uint8)
        return values, nearest, fits

    @staticmethod
    def query(points, rows, R, first=0, skipped=()):
        """(distances (P,), nearest (P,), towards (P, 2)) of points (P, 2) over `rows` numbered from `first`."""
        points = np.asarray(points, F).reshape(-1, 2)
        rows = np.asarray(rows, F).reshape(-1, 4)
        x, y = points[:, 0].copy(), points[:, 1].copy()
        bd, bi, bt = clear_rule.winner(x, y, rows, R, first, skipped)
        won = bi != NONE
        d = np.where(won, np.sqrt(bd), INF).astype(F)
        row = rows[np.where(won, bi - first, 0)] if len(rows) else np.zeros((len(x), 4), F)
        vx, vy, px, py = row[:, 2] - row[:, 0], row[:, 3] - row[:, 1], x - row[:, 0], y - row[:, 1]
        with np.errstate(all='ignore'):
            dx, dy = px - bt*vx, py - bt*vy
            towards = np.stack([-dx/d, -dy/d], 1).astype(F)
        towards[~(won & (d > 0))] = 0
        return d, np.where(won, bi, -1).astype(np.int32), towards


def _aligned(a, dtype=np.int32, align=16):
    a = np.asarray(a, dtype)
    raw = np.zeros(a.nbytes + align, np.uint8)
    off = (-raw.ctypes.data) % align
    out = raw[off:off + a.nbytes].view(dtype).reshape(a.shape)
    out[...] = a
    return out


def _max_tiles(geom):
    return max([((int(g[2]) + 15)//16)*((int(g[3]) + 15)//16) for g in geom if g[2] > 0 and g[3] > 0], default=1)


class _Host:
    """ms_host_nav_clearance on one grid of host arrays; the outputs start as sentinels."""

    def __init__(self, geoms, walls, cell=CELL, clearance=RADIUS):
        from megastep_amd import _lib
        self.geom = _aligned(np.asarray(geoms, np.int32).reshape(-1, 4))
        counts = [int(g[2])*int(g[3]) if g[2] > 0 and g[3] > 0 else 0 for g in self.geom]
        self.starts = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        self.N, self.cell = len(self.geom), cell
        self.free = np.zeros(max(int(self.starts[-1]), 1), np.uint8)
        self.env_walls = [np.asarray(w, F).reshape(-1, 4) for w in walls]
        self.walls = np.ascontiguousarray(np.concatenate(self.env_walls + [np.zeros((1, 4), F)]))
        self.wall_starts = np.concatenate([[0], np.cumsum([len(w) for w in self.env_walls])]).astype(np.int64)
        framed = max([(int(g[2]) + 2)*(int(g[3]) + 2) for g in self.geom if g[2] > 0 and g[3] > 0], default=0)
        self.grid = _lib.MsNavGrid(self.N, cell, clearance, self.geom.ctypes.data, self.starts.ctypes.data, framed, self.free.ctypes.data)
        self.h = _lib.lib()

    def field(self, R, radii=(), flags=TILE_WAVE, mask=None, before=None, expect=0):
        from megastep_amd import _lib
        size, K = max(int(self.starts[-1]), 1), len(radii)
        out = before if before is not None else dict(values=np.full(size, -3, F), nearest=np.full(size, -7, np.int32), fits=np.full(max(K, 1)*size, 9, np.uint8))
        out = {k: np.ascontiguousarray(v).copy() for k, v in out.items()}
        mask = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        spec = _lib.MsNavClearance(float(R), K, (ctypes.c_float*8)(*radii), _max_tiles(self.geom), None if mask is None else mask.ctypes.data,
                                   out['values'].ctypes.data, out['nearest'].ctypes.data, out['fits'].ctypes.data if K else None)
        assert self.h.ms_host_nav_clearance(ctypes.byref(self.grid), ctypes.byref(spec), self.walls.ctypes.data, self.wall_starts.ctypes.data, flags) == expect
        pairs = ctypes.c_longlong()
        out['folds'] = self.h.ms_host_nav_clear_folds(ctypes.byref(pairs))
        out['pairs'] = pairs.value
        return out

    def rule(self, R, radii=()):
        size, K = max(int(self.starts[-1]), 1), len(radii)
        out = dict(values=np.full(size, -3, F), nearest=np.full(size, -7, np.int32), fits=np.full(max(K, 1)*size, 9, np.uint8))
        for n in range(self.N):
            s, cells = int(self.starts[n]), int(self.starts[n + 1] - self.starts[n])
            if cells == 0:
                continue
            values, nearest, fits = clear_rule.field(self.env_walls[n], tuple(int(v) for v in self.geom[n]), self.cell, R, radii)
            out['values'][s:s + cells], out['nearest'][s:s + cells] = values.reshape(-1), nearest.reshape(-1)
            for k in range(K):
                out['fits'][K*s + k*cells:][:cells] = fits[k].reshape(-1)
        return out


def same(got, want, keys=('values', 'nearest', 'fits')):
    for key in keys:
        a, b = np.asarray(got[key]), np.asarray(want[key])
        a, b = (bits(a), bits(b)) if a.dtype == F else (a, b)
        assert np.array_equal(a, b), (key, int((a != b).sum()))


def query_host(points, rows, R, n_agents=1, n_model=1, with_agents=False, skip=None, mask=None, flags=0, before=None, expect=0):
    """ms_host_nav_clear_query on host arrays: points (N, P, 2), rows a list of (L_n, 4) per env (agent rows first)."""
    from megastep_amd import _lib
    points = np.ascontiguousarray(points, F)
    N, P = points.shape[:2]
    env_rows = [np.asarray(r, F).reshape(-1, 4) for r in rows]
    flat = np.ascontiguousarray(np.concatenate(env_rows + [np.zeros((1, 4), F)]))
    starts = np.concatenate([[0], np.cumsum([len(r) for r in env_rows])]).astype(np.int64)
    out = before if before is not None else dict(distances=np.full((N, P), -3, F), nearest=np.full((N, P), -7, np.int32), towards=np.full((N, P, 2), 5, F))
    out = {k: np.ascontiguousarray(v).copy() for k, v in out.items()}
    skip = None if skip is None else np.ascontiguousarray(skip, np.int32)
    mask = None if mask is None else np.ascontiguousarray(mask, np.uint8)
    spec = _lib.MsNavClearQuery(N, P, points.ctypes.data, None if skip is None else skip.ctypes.data, float(R), None if mask is None else mask.ctypes.data,
                                out['distances'].ctypes.data, out['nearest'].ctypes.data, out['towards'].ctypes.data)
    status = _lib.lib().ms_host_nav_clear_query(ctypes.byref(spec), flat.ctypes.data, starts.ctypes.data, n_agents, n_model, int(with_agents), flags)
    assert status == expect
    return out


def query_rule(points, rows, R, n_agents=1, n_model=1, with_agents=False, skip=None):
    points = np.asarray(points, F)
    N, P = points.shape[:2]
    out = dict(distances=np.zeros((N, P), F), nearest=np.zeros((N, P), np.int32), towards=np.zeros((N, P, 2), F))
    af = n_agents*n_model
    for n in range(N):
        r = np.asarray(rows[n], F).reshape(-1, 4)
        who = np.full(P, -1) if skip is None or not with_agents else np.where((np.asarray(skip[n]) >= 0) & (np.asarray(skip[n]) < n_agents), skip[n], -1)
        for s in np.unique(who):
            sel = who == s
            skipped = set(range(s*n_model, (s + 1)*n_model)) if s >= 0 else ()
            d, l, t = clear_rule.query(points[n, sel], r if with_agents else r[af:], R, 0 if with_agents else af, skipped)
            out['distances'][n, sel], out['nearest'][n, sel], out['towards'][n, sel] = d, l, t
    return out


def plan_host(n=4, cell=CELL, clearance=RADIUS):
    gs = list(plans(n)) + list(plans(n, oblique=True))
    walls = [np.asarray(g['walls'], F) for g in gs]
    return _Host([nav_rule.geometry(w, cell) for w in walls], walls, cell, clearance), walls


@pytest.fixture(scope='module')
def planned():
    return plan_host()


# ---------------------------------------------------------------------------------------------------------------------
# the rule against the host instantiation, and the culls against brute force
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('R', RANGES)
def test_the_host_instantiation_equals_the_rule_on_floorplans(planned, R):
    """4 plain and 4 oblique plans, brute force and both culls: values, nearest and three fits as bits."""
    host, _ = planned
    radii = tuple(r for r in (RADIUS, .2, .3) if F(r) <= F(R))
    want = host.rule(R, radii)
    finite = np.isfinite(want['values'][:int(host.starts[-1])])
    assert {.3: finite.mean() < .8, 2.: 0 < (~finite).sum() and finite.mean() > .5, 50.: finite.all()}[R]
    for flags in (BRUTE, TILE, TILE_WAVE):
        same(host.field(R, radii, flags), want)


@pytest.mark.parametrize('cell,clearance', CELLS)
def test_the_host_instantiation_equals_the_rule_at_other_cell_widths(cell, clearance):
    host, _ = plan_host(1, cell, clearance)
    want = host.rule(2., (clearance, .3))
    for flags in (BRUTE, TILE, TILE_WAVE):
        same(host.field(2., (clearance, .3), flags), want)


def strained_worlds():
    """[(geom, walls (L, 4))] at CELL = .125 (centres ((origin + k) + .5)/8: exact) and R = .5, each made to strain a cull; a few
    random walls in each so that every tile has work."""
    rng = np.random.RandomState(5)

    def some(lo, hi, k=12):
        a = rng.uniform(lo, hi, (k, 2))
        return np.concatenate([a, a + rng.normal(size=(k, 2))*.7], 1)

    corner = 15.5*.125                  # the last centre of tile (0, 0), both axes
    out = []
    # a wall exactly R from a tile's corner centre, one an ulp nearer and one an ulp further
    walls = [[corner + .5, 0., corner + .5, 5.], [np.nextafter(F(corner + .5), F(0)), 0., np.nextafter(F(corner + .5), F(0)), 5.],
             [np.nextafter(F(corner + .5), F(9)), 0., np.nextafter(F(corner + .5), F(9)), 5.], [0., corner + .5, 5., corner + .5]]
    out.append(((0, 0, 40, 40), np.array(walls)))
    # a wall whose bounding box touches the grown tile box at a corner; a long oblique wall passing the tile diagonally just outside R
    far = corner + .5
    walls = [[far, far, far + 1., far + 1.], [far + .5/2**.5 + 1e-4 + 3., far - .5/2**.5 - 3., far - .5/2**.5 - 3., far + .5/2**.5 + 1e-4 + 3.],
             [corner + (.5 + 1e-4)*2**.5 + 4., corner - 4., corner - 4., corner + (.5 + 1e-4)*2**.5 + 4.],
             [corner + (.5 - 1e-4)*2**.5 + 4., corner - 4., corner - 4., corner + (.5 - 1e-4)*2**.5 + 4.]]
    out.append(((0, 0, 48, 48), np.concatenate([np.array(walls), some(0, 6)])))
    # zero-length walls, duplicated walls (the tie goes to the least index), a wall through centres (d == 0)
    a = some(0, 4, 6)
    walls = np.concatenate([[[1.0625, 1.0625, 1.0625, 1.0625], [2., 2., 2., 2.]], a, a[::-1], a[:3], [[.0625, .5625, 3.9375, .5625]]])
    out.append(((0, 0, 33, 33), walls))
    # NaN and infinite rows among good ones: never a winner, the rest unaffected
    walls = some(0, 4, 16)
    for k, (row, coord, bad) in enumerate([(1, 0, np.nan), (3, 2, np.inf), (5, 1, -np.inf), (7, 3, np.nan), (9, 0, np.inf)]):
        walls[row, coord] = bad
        if k % 2:
            walls[row, (coord + 2) % 4] = np.nan
    out.append(((0, 0, 32, 32), walls))
    # coordinates near 30 m
    out.append(((232, 236, 47, 31), some(29.2, 34.5, 20)))
    # grids 1, 15, 16 and 17 cells beyond a multiple of 16
    for nx, ny in ((1, 15), (17, 31), (32, 33), (16, 1), (49, 16)):
        out.append(((-3, 2, nx, ny), some(-.5, 4., 10)))
    # more static rows than one LDS list holds, all near one tile: the fold-and-empty path
    a = rng.uniform(.2, 1.8, (1100, 2))
    out.append(((0, 0, 20, 18), np.concatenate([a, a + rng.normal(size=(1100, 2))*.05], 1)))
    return out


def test_the_culls_change_no_bit_on_worlds_made_to_strain_them():
    from megastep_amd import _lib
    worlds = strained_worlds()
    host = _Host([g for g, _ in worlds], [w for _, w in worlds])
    assert host.wall_starts[-1] - host.wall_starts[-2] > _lib.lib().ms_host_nav_clear_chunk()
    radii = (RADIUS, .3, .5)
    want = host.rule(.5, radii)
    brute = host.field(.5, radii, BRUTE)
    same(brute, want)
    for flags in (TILE, TILE_WAVE):
        got = host.field(.5, radii, flags)
        same(got, brute)
        assert got['folds'] < brute['folds'] == brute['pairs']
    # the wall exactly R away IS the winner of the corner centre (d2 == R*R), the one an ulp nearer wins over it, the ulp further never
    values, nearest = want['values'][:1600].reshape(40, 40), want['nearest'][:1600].reshape(40, 40)
    assert nearest[0, 15] == 1 and values[0, 15] < F(.5) and (nearest[:16, :16] != 2).all()
    world = clear_rule.field(worlds[0][1][[0, 3]], worlds[0][0], CELL, .5)
    assert world[0][15, 15] == F(.5) and world[1][15, 15] == 0          # (both exactly R away: the lower row)
    # duplicates: never the later copy
    s = int(host.starts[2])
    assert not np.isin(want['nearest'][s:s + 33*33], np.arange(8, 17)).any()
    # NaN and inf rows are nobody's winner
    s = int(host.starts[3])
    assert not np.isin(want['nearest'][s:s + 32*32], (1, 3, 5, 7, 9)).any() and np.isfinite(want['values'][s:s + 32*32]).any()


def test_the_culls_do_cull_on_floorplans(planned):
    host, _ = planned
    shares = {}
    for flags in (BRUTE, TILE, TILE_WAVE):
        out = host.field(2., (), flags)
        shares[flags] = out['folds']/out['pairs']
    print(f'rows folded per cell, share of all (cell, row) pairs at R = 2: tile cull {shares[TILE]:.3f}, tile and wave culls {shares[TILE_WAVE]:.3f}')
    assert shares[BRUTE] == 1. and shares[TILE_WAVE] <= shares[TILE] < 1.


def test_a_masked_env_keeps_its_stores(planned):
    host, _ = planned
    full = host.field(2., (RADIUS,))
    mask = np.arange(host.N) % 2
    got = host.field(.3, (RADIUS,), mask=mask, before={k: full[k] for k in ('values', 'nearest', 'fits')})
    want = host.rule(.3, (RADIUS,))
    for n in range(host.N):
        s, e = int(host.starts[n]), int(host.starts[n + 1])
        ref = want if mask[n] else full
        assert np.array_equal(bits(got['values'][s:e]), bits(ref['values'][s:e])) and np.array_equal(got['fits'][s:e], ref['fits'][s:e])


def test_fits_are_the_free_bytes_of_the_existing_rule(planned):
    host, walls = planned
    radii = (RADIUS, .2, .3)
    got = host.field(2., radii)
    for n in (0, 5):
        s, cells = int(host.starts[n]), int(host.starts[n + 1] - host.starts[n])
        geom = tuple(int(v) for v in host.geom[n])
        for k, r in enumerate(radii):
            free = nav_rule.free(walls[n], geom, CELL, r)
            assert np.array_equal(got['fits'][3*s + k*cells:][:cells], free.reshape(-1).astype(np.uint8)), (n, r)


# The largest deviation of the numpy rule's values from the float64 distance on these plans at R = 2, measured on the CPU:
# 1.04e-6 m, an ulp of a coordinate near 12 m (test_the_distances_against_float64 prints it).  Four times that is the bound: a later seed's plans may round worse.
MEASURED_DEVIATION = 1.04e-6
FLOAT64_BOUND = 4*MEASURED_DEVIATION


def test_the_distances_against_float64(planned):
    host, walls = planned
    R = 2.
    got = host.field(R, ())
    rule = host.rule(R, ())
    worst_rule = worst = 0.
    for n in range(host.N):
        s, cells = int(host.starts[n]), int(host.starts[n + 1] - host.starts[n])
        x, y = nav_rule.centres(tuple(int(v) for v in host.geom[n]), CELL)
        pts = np.stack(np.broadcast_arrays(x[None, :], y[:, None]), -1).reshape(-1, 2)
        exact = _distance_to_walls(pts, walls[n])
        v = got['values'][s:s + cells]
        won = np.isfinite(v)
        assert won.any()
        worst = max(worst, float(np.abs(v[won].astype(np.float64) - exact[won]).max()))
        worst_rule = max(worst_rule, float(np.abs(rule['values'][s:s + cells][won].astype(np.float64) - exact[won]).max()))
        assert (exact[~won] > R*(1 - 1e-5)).all()
    print(f'largest deviation from float64: the numpy rule {worst_rule:.3g} m, the host instantiation {worst:.3g} m')
    assert worst <= FLOAT64_BOUND


# ---------------------------------------------------------------------------------------------------------------------
# the point query
# ---------------------------------------------------------------------------------------------------------------------
def test_the_query_equals_the_rule_and_the_field(planned):
    """2000 random points per plan, cell centres among them; one stand-in agent row in front of the walls, not met."""
    host, walls = planned
    rng = np.random.RandomState(2)
    points, rows = [], []
    for n in range(host.N):
        geom = tuple(int(v) for v in host.geom[n])
        x, y = nav_rule.centres(geom, CELL)
        lo, hi = walls[n].reshape(-1, 2).min(0) - 1., walls[n].reshape(-1, 2).max(0) + 1.
        p = (lo + rng.uniform(0, 1, (2000, 2))*(hi - lo)).astype(F)
        cells = rng.randint(0, geom[2]*geom[3], 600)
        p[:600] = np.stack([x[cells % geom[2]], y[cells // geom[2]]], 1)
        p[600] = [np.nan, 1.]
        p[601] = [1., np.nan]
        points.append(p)
        rows.append(np.concatenate([[[0., 0., 1e-3, 0.]], walls[n].reshape(-1, 4)]))
    points = np.stack(points)
    for R in (.3, 2.):
        want = query_rule(points, rows, R)
        for flags in (0, 1):
            same(query_host(points, rows, R, flags=flags), want, ('distances', 'nearest', 'towards'))
        assert (want['nearest'][:, 600:602] == -1).all() and np.isinf(want['distances'][:, 600:602]).all()
        field = host.rule(R)
        for n in range(host.N):
            geom = tuple(int(v) for v in host.geom[n])
            x, y = nav_rule.centres(geom, CELL)
            j, i = np.searchsorted(x, points[n, :600, 0]), np.searchsorted(y, points[n, :600, 1])
            at = int(host.starts[n]) + i*geom[2] + j
            assert np.array_equal(bits(want['distances'][n, :600]), bits(field['values'][at]))
            assert np.array_equal(want['nearest'][n, :600], np.where(field['nearest'][at] >= 0, field['nearest'][at] + 1, -1))
        norm = np.linalg.norm(want['towards'].astype(np.float64), axis=-1)
        assert (np.abs(norm[np.isfinite(want['distances']) & (want['distances'] > 0)] - 1) < 1e-6).all()


def _bodies(positions, half=.1):
    """Four rows a body: the square of side 2*half round each position."""
    rows = []
    for x, y in positions:
        c = [(x - half, y - half), (x + half, y - half), (x + half, y + half), (x - half, y + half)]
        rows += [[*c[k], *c[(k + 1) % 4]] for k in range(4)]
    return np.array(rows, F)


def test_the_query_meets_the_other_agents_and_skips_its_own():
    box = np.array([[0, 0, 4, 0], [4, 0, 4, 4], [4, 4, 0, 4], [0, 4, 0, 0]], F)
    positions = np.array([[[1., 1.], [1.2, 1.], [3., 3.]],               # agents 0 and 1 touch (their squares share a side)
                          [[2., 2.], [2., 3.9], [.5, .5]]], F)
    rows = [np.concatenate([_bodies(p), box]) for p in positions]
    own = np.arange(3)[None].repeat(2, 0)
    for skip, name in ((own, 'own'), (np.full((2, 3), -1), 'none'), (np.array([[7, -5, 1], [0, 3, 2]]), 'mixed')):
        want = query_rule(positions, rows, 2., 3, 4, True, skip)
        for flags in (0, 1):
            same(query_host(positions, rows, 2., 3, 4, True, skip, flags=flags), want, ('distances', 'nearest', 'towards'))
        if name == 'own':
            assert (want['nearest']//4 != own).all()                    # nobody's nearest is its own body
            assert want['nearest'][0, 0]//4 == 1 and want['distances'][0, 0] == F(1.2) - F(.1) - F(1.)
            assert want['nearest'][1, 1] == 12 + 2 and abs(want['distances'][1, 1] - .1) < 1e-6    # the box's top wall
        if name == 'none':
            # everybody's nearest is its own body - but for agent 1 of env 0, whose body shares a side with agent 0's: a lower row
            touching = np.zeros((2, 3), bool)
            touching[0, 1] = True
            assert (want['nearest']//4 == np.where(touching, 0, own)).all() and np.allclose(want['distances'], .1, atol=1e-6)
    # without agents no body is met, whatever skip says
    same(query_host(positions, rows, 2., 3, 4, False, own), query_rule(positions, rows, 2., 3, 4, False), ('distances', 'nearest', 'towards'))
    # a point on a wall: d == 0 and towards == (0, 0); one out of range: +inf, -1, (0, 0)
    pts = np.array([[[4., 2.], [2., 0.], [2., 2.]], [[0., 0.], [9., 9.], [3., 4.]]], F)
    got = query_host(pts, rows, .5, 3, 4, False)
    same(got, query_rule(pts, rows, .5, 3, 4, False), ('distances', 'nearest', 'towards'))
    assert got['distances'][0, 0] == 0 and (got['towards'][0, 0] == 0).all() and got['nearest'][0, 0] == 13
    assert np.isinf(got['distances'][1, 1]) and got['nearest'][1, 1] == -1 and (got['towards'][1, 1] == 0).all()
    # a masked point keeps its outputs
    before = dict(distances=np.full((2, 3), 42, F), nearest=np.full((2, 3), 42, np.int32), towards=np.full((2, 3, 2), 42, F))
    mask = np.array([[1, 0, 1], [0, 0, 1]])
    kept = query_host(pts, rows, .5, 3, 4, False, mask=mask, before=before)
    assert (kept['distances'][mask == 0] == 42).all() and np.array_equal(kept['nearest'][mask == 1], got['nearest'][mask == 1])


def test_the_reduction_is_order_free():
    """More rows than lanes, many ties (every wall four times): the rows dealt to 64 bests and merged give the serial fold's bits."""
    rng = np.random.RandomState(9)
    a = rng.uniform(0, 4, (90, 2))
    walls = np.concatenate([a, a + rng.normal(size=(90, 2))], 1).astype(F)
    rows = [np.concatenate([walls, walls[::-1], walls, walls[::3]])]
    points = rng.uniform(-1, 5, (1, 500, 2)).astype(F)
    serial = query_host(points, rows, 1.5, 1, 1, True)
    same(query_host(points, rows, 1.5, 1, 1, True, flags=1), serial, ('distances', 'nearest', 'towards'))
    same(serial, query_rule(points, rows, 1.5, 1, 1, True), ('distances', 'nearest', 'towards'))
    assert (serial['nearest'] < 90).all()


# ---------------------------------------------------------------------------------------------------------------------
# the C-ABI and the Python calls
# ---------------------------------------------------------------------------------------------------------------------
NEW = ('ms_nav_clearance', 'ms_nav_clear_query')
HOOKS = ('ms_host_nav_clearance', 'ms_host_nav_clear_folds', 'ms_host_nav_clear_chunk', 'ms_host_nav_clear_query', 'ms_debug_nav_clear_cull')


def test_the_header_declares_the_calls_and_the_abi_version_stays():
    from megastep_amd import _lib
    public = declared_symbols(('megastep_hip.h',))
    assert set(NEW) <= set(public) and not set(HOOKS) & set(public)
    assert set(HOOKS) <= set(declared_symbols(('megastep_hip_test.h',)))
    assert set(NEW + HOOKS) <= set(_lib.SYMBOLS)
    text = open(os.path.join(ROOT, 'include', 'megastep_hip.h')).read()
    assert int(re.search(r'#define MS_ABI_VERSION (\d+)', text).group(1)) == _lib.ABI_VERSION == 17
    handle = _lib.lib()
    assert all(hasattr(handle, name) for name in NEW + HOOKS)
    assert handle.ms_host_nav_clear_chunk() == 1024


def test_the_mirrors_have_the_c_layout():
    import subprocess
    import tempfile
    from megastep_amd import _lib
    names = ('MsNavClearance', 'MsNavClearQuery')
    exprs = [e for name in names for e in [f'sizeof({name})'] + [f'offsetof({name}, {f})' for f, _ in getattr(_lib, name)._fields_]]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "megastep_hip.h"\nint main(){' + ''.join(f'printf("%zu ", (size_t){e});' for e in exprs) + '}'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, 't.c'), 'w').write(src)
        subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), os.path.join(d, 't.c'), '-o', os.path.join(d, 't')])
        got = list(map(int, subprocess.check_output([os.path.join(d, 't')]).split()))
    want = [v for name in names for v in [ctypes.sizeof(getattr(_lib, name))] + [getattr(getattr(_lib, name), f).offset for f, _ in getattr(_lib, name)._fields_]]
    assert got == want
    assert [f for f, _ in _lib.MsNavClearance._fields_] == ['max_range', 'n_radii', 'radii', 'max_tiles', 'mask', 'values', 'nearest', 'fits']


def test_bad_arguments_are_refused_before_any_launch():
    from megastep_amd import _lib
    h = _lib.lib()
    ref = ctypes.byref
    # NULLs and zeroed structs
    assert h.ms_nav_clearance(None, None, None, None) == -1 and h.ms_nav_clear_query(None, None, None, None) == -1
    assert h.ms_nav_clearance(ref(_lib.MsScenery()), ref(_lib.MsNavGrid()), ref(_lib.MsNavClearance()), None) == -1
    assert h.ms_nav_clear_query(ref(_lib.MsScenery()), ref(_lib.MsAgents()), ref(_lib.MsNavClearQuery()), None) == -1
    assert h.ms_host_nav_clearance(None, None, None, None, 0) == -1 and h.ms_host_nav_clear_query(None, None, None, 1, 1, 0, 0) == -1
    fake = 64                                       # (never dereferenced: every call below fails its checks first)
    grid = _lib.MsNavGrid(n_envs=2, cell=.125, clearance=.106, geom=fake, starts=fake, max_framed=100, free_cells=fake)
    scenery = _lib.MsScenery(n_envs=2, n_agents=1, n_model=1, lines_vals=fake, lines_widths=fake, lines_starts=fake, model=fake)
    other = _lib.MsScenery(n_envs=3, n_agents=1, n_model=1, lines_vals=fake, lines_widths=fake, lines_starts=fake, model=fake)
    radii = lambda *r: (ctypes.c_float*8)(*r)
    good = dict(max_range=2., n_radii=2, radii=radii(.1, 2.), max_tiles=4, mask=None, values=fake, nearest=fake, fits=fake)
    bad_ones = (dict(max_range=0.), dict(max_range=-1.), dict(max_range=float('inf')), dict(max_range=float('nan')), dict(n_radii=-1), dict(n_radii=9),
                dict(radii=radii(.1, 0.)), dict(radii=radii(-1., 1.)), dict(radii=radii(.1, float(np.nextafter(F(2), F(3))))),
                dict(radii=radii(float('nan'), 1.)), dict(values=None), dict(fits=None), dict(n_radii=0), dict(max_tiles=0), dict(values=66), dict(nearest=66))
    for bad in bad_ones:
        spec = _lib.MsNavClearance(**{**good, **bad})
        assert h.ms_nav_clearance(ref(scenery), ref(grid), ref(spec), None) == -1, bad
        assert h.ms_host_nav_clearance(ref(grid), ref(spec), fake, fake, TILE) == -1, bad
    spec = _lib.MsNavClearance(**good)
    assert h.ms_nav_clearance(None, ref(grid), ref(spec), None) == -1 and h.ms_nav_clearance(ref(scenery), None, ref(spec), None) == -1
    assert h.ms_nav_clearance(ref(scenery), ref(grid), None, None) == -1 and h.ms_nav_clearance(ref(other), ref(grid), ref(spec), None) == -1
    assert h.ms_host_nav_clearance(ref(grid), ref(spec), None, fake, TILE) == -1 and h.ms_host_nav_clearance(ref(grid), ref(spec), fake, None, TILE) == -1
    assert h.ms_host_nav_clearance(ref(grid), ref(spec), fake, fake, 3) == -1 and h.ms_host_nav_clearance(ref(grid), ref(spec), fake, fake, -1) == -1
    good = dict(n_envs=2, n_points=3, points=fake, skip=None, max_range=2., mask=None, distances=fake, nearest=fake, towards=fake)
    bad_ones = (dict(n_envs=0), dict(n_envs=3), dict(n_points=0), dict(points=None), dict(distances=None, nearest=None, towards=None), dict(max_range=0.),
                dict(max_range=float('inf')), dict(max_range=float('nan')), dict(points=68), dict(towards=68), dict(skip=66), dict(distances=66))
    agents = _lib.MsAgents(angles=fake, positions=fake)
    for bad in bad_ones:
        spec = _lib.MsNavClearQuery(**{**good, **bad})
        assert h.ms_nav_clear_query(ref(scenery), None, ref(spec), None) == -1, bad
        assert h.ms_nav_clear_query(ref(scenery), ref(agents), ref(spec), None) == -1, bad
        if 'n_envs' not in bad or bad['n_envs'] < 1:
            assert h.ms_host_nav_clear_query(ref(spec), fake, fake, 1, 1, 0, 0) == -1, bad
    spec = _lib.MsNavClearQuery(**good)
    assert h.ms_nav_clear_query(None, None, ref(spec), None) == -1 and h.ms_nav_clear_query(ref(scenery), None, None, None) == -1
    assert h.ms_nav_clear_query(ref(scenery), ref(_lib.MsAgents()), ref(spec), None) == -1          # (agents without poses)
    assert h.ms_nav_clear_query(ref(scenery), ref(_lib.MsAgents(angles=fake, positions=68)), ref(spec), None) == -1
    assert h.ms_host_nav_clear_query(ref(spec), None, fake, 1, 1, 0, 0) == -1 and h.ms_host_nav_clear_query(ref(spec), fake, fake, 0, 1, 0, 0) == -1
    assert h.ms_host_nav_clear_query(ref(spec), fake, fake, 1, 1, 0, 2) == -1
    assert h.ms_debug_nav_clear_cull(3) == -1 and h.ms_debug_nav_clear_cull(-2) == -1 and h.ms_debug_nav_clear_cull(-1) == 0


def test_the_python_calls_refuse_what_they_cannot_do():
    from megastep_amd import core, cuda, nav, scene, toys
    assert cuda.clearance_fields is nav.clearance_fields and cuda.clearance is nav.clearance and cuda.ClearanceFields is nav.ClearanceFields
    geom = np.array([[0, 0, 8, 8], [0, 0, 8, 8]], np.int32)
    starts = np.array([0, 64, 128], np.int64)
    grid = cuda.NavGrid(torch.as_tensor(geom), torch.as_tensor(starts), torch.ones(128, dtype=torch.uint8), CELL, RADIUS, geom, starts)
    scenery = scene.scenery([toys.box(), toys.box()], 1, device='cpu', bake=False)
    with pytest.raises(RuntimeError, match='GPU'):
        cuda.clearance_fields(grid, scenery)        # (CPU tensors)
    points = torch.zeros((2, 3, 2))
    with pytest.raises(RuntimeError, match='GPU'):
        cuda.clearance(scenery, points)
    agents = core._init_agents(2, 1, 'cpu')
    with pytest.raises(RuntimeError, match='GPU'):
        cuda.clearance(scenery, points, agents=agents, skip=torch.zeros((2, 3), dtype=torch.int64))
    for bad in (0, -1., float('inf'), float('nan'), 'far'):
        with pytest.raises(RuntimeError, match='max_range'):
            cuda.clearance_fields(grid, scenery, max_range=bad)
        with pytest.raises(RuntimeError, match='max_range'):
            cuda.clearance(scenery, points, max_range=bad)
    for bad in ((0.,), (-.1,), (2.5,), (float('nan'),), tuple([.1]*9)):
        with pytest.raises(RuntimeError, match='radi'):
            cuda.clearance_fields(grid, scenery, radii=bad)
    with pytest.raises(RuntimeError, match='scenery'):
        cuda.clearance_fields(grid, scene.scenery([toys.box()], 1, device='cpu', bake=False))
    for bad in (torch.zeros((3, 3, 2)), torch.zeros((2, 3, 3)), torch.zeros((2, 0, 2))):
        with pytest.raises(RuntimeError, match=r'\(N, P, 2\)'):
            cuda.clearance(scenery, bad)
    with pytest.raises(RuntimeError, match='skip goes with agents'):
        cuda.clearance(scenery, points, skip=torch.zeros((2, 3), dtype=torch.int32))
    with pytest.raises(RuntimeError, match='skip'):
        cuda.clearance(scenery, points, agents=agents, skip=torch.zeros((2, 2), dtype=torch.int32))
    with pytest.raises(RuntimeError, match='mask'):
        cuda.clearance(scenery, points, mask=torch.ones((2, 2), dtype=torch.bool))
    # a ClearanceFields is a float layer of one store as it is; its nav_grid needs fits, a k in range and a cell that fits the radius
    clear = nav.ClearanceFields(grid, scenery, 2., (RADIUS, .05), torch.ones(128), None, torch.ones(256, dtype=torch.uint8))
    layer = cuda.cell_layer(clear)
    assert layer.values is clear.values and layer.n_fields == 1 and layer.is_float
    assert cuda.cell_layer(clear.fits, n_fields=2).n_fields == 2
    assert clear._max_tiles == 1 and clear.image(1).shape == (8, 8) and clear.fits_image(1, 1).dtype == torch.bool
    with pytest.raises(RuntimeError, match='1.4'):
        clear.nav_grid(1)
    with pytest.raises(RuntimeError, match='k must'):
        clear.nav_grid(2)
    with pytest.raises(RuntimeError, match='nearest'):
        clear.nearest_image(0)
    clear.fits[64 + 64 + 3] = 0                      # env 1 (stores at 2*64), store 0, cell 3
    sub = clear.nav_grid(0)
    assert sub.clearance == RADIUS and sub.geom is grid.geom and sub.free[64 + 3] == 0 and int(sub.free.sum()) == 127


# ---------------------------------------------------------------------------------------------------------------------
# modules.Proximity on a stand-in for cuda.clearance
# ---------------------------------------------------------------------------------------------------------------------
# to_local_frame forms a = fl(fl(pi/180)*angle), s = sinf(a), c = cosf(a), then c*x + s*y and -s*x + c*y.  With |angle| <= 180:
# |a| <= pi and a is off pi/180*angle by at most 2 roundings, pi*2^-23; sinf and cosf add an ulp of 1 at most, 2^-24 - so s and c
# are each off by at most pi*2^-23 + 2^-24.  For a unit vector |x| + |y| <= sqrt(2), so the rotated component is off by
# sqrt(2)*(pi*2^-23 + 2^-24) for s and c, plus three roundings of values of size <= sqrt(2): 3*sqrt(2)*2^-24.  In all
# sqrt(2)*(pi + .5 + 1.5)*2^-23 = 7.3 * 2^-23: eight binary32 ulps of 1.
ROTATION_BOUND = 8*2.**-23


def test_proximity_on_a_stand_in(monkeypatch):
    from megastep_amd import cuda, modules, spaces
    rng = np.random.RandomState(4)
    N, A = 5, 3
    theta = rng.uniform(0, 2*np.pi, (N, A))
    towards = torch.as_tensor(np.stack([np.cos(theta), np.sin(theta)], -1).astype(F))
    distances = torch.as_tensor(rng.uniform(0, 1.5, (N, A)).astype(F))
    distances[0, 0], towards[0, 0] = float('inf'), 0.
    distances[1, 1], towards[1, 1] = 0., 0.
    angles = torch.as_tensor(rng.uniform(-180, 180, (N, A)).astype(F))
    angles[2] = torch.tensor([0., 90., -180.])
    calls = []

    def fake(scenery, points, max_range=2., agents=None, skip=None, mask=None, out=None):
        calls.append(dict(points=points, max_range=max_range, agents=agents, skip=skip, out=out))
        return out if out is not None else cuda.Clearance(distances, torch.zeros((N, A), dtype=torch.int32), towards)

    monkeypatch.setattr(cuda, 'clearance', fake)
    agents = type('Agents', (), dict(positions=torch.zeros((N, A, 2)), angles=angles))()
    stand_in = type('Core', (), dict(n_envs=N, n_agents=A, device='cpu', scenery=object(), agents=agents))()
    for others in (True, False):
        prox = modules.Proximity(stand_in, max_range=1.5, others=others)
        assert isinstance(prox.space, spaces.MultiVector) and prox.space.shape == spaces.MultiVector(A, 3).shape
        obs = prox()
        again = prox()
        assert obs.shape == (N, A, 3) and obs.dtype == torch.float32 and torch.equal(obs, again)
        first, second = calls[-2:]
        assert first['out'] is None and second['out'] is prox.reading and first['points'] is agents.positions and first['max_range'] == 1.5
        if others:
            assert first['agents'] is agents and torch.equal(first['skip'], torch.arange(A, dtype=torch.int32).expand(N, A))
        else:
            assert first['agents'] is None and first['skip'] is None
        assert torch.equal(obs[..., 0], (distances/1.5).clamp(max=1.)) and obs[0, 0, 0] == 1 and obs[1, 1, 0] == 0
        a = np.deg2rad(angles.numpy().astype(np.float64))
        x, y = towards[..., 0].numpy().astype(np.float64), towards[..., 1].numpy().astype(np.float64)
        want = np.stack([np.cos(a)*x + np.sin(a)*y, -np.sin(a)*x + np.cos(a)*y], -1)
        assert np.abs(obs[..., 1:].numpy().astype(np.float64) - want).max() <= ROTATION_BOUND
        assert (obs[0, 0, 1:] == 0).all() and (obs[1, 1, 1:] == 0).all()
        assert torch.equal(obs[2, 0, 1:], towards[2, 0])                 # (heading 0: the agent's frame is the world's)
