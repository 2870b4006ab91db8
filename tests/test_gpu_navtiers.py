"""Every instantiation of the relaxation (`nav_relax_kernel`: three LDS tiers, each single-goal and seeded) at its edge: an env
of exactly `cuda.FIELD_CAPACITY[which]` framed cells and one a column wider, `cuda.distance_fields`, `DistanceFields.at` and
`cuda.seeded_fields` equal AS BITS to the numpy rules (tests/test_navfield_host.nav_rule, tests/test_navseed_host.seed_rule).
A launch takes the tier of its largest env, so every env of a launch runs that tier's code: next to the boundary env ride a
9 x 7 env, envs one cell wide and one cell high (row pitches of 3 and of 302), a single cell, an env that is all blocked and
one without cells, each exact against the rule under every tier's thread count.

What each case launches, by the asserted `grid._max_framed`:
  110 x 71 = 8176     the 40 KiB instantiations (512 threads), every env in LDS
  111 x 71 = 8249     the 80 KiB ones (1024 threads), every env in LDS
  130 x 122 = 16368   the 80 KiB ones, every env in LDS
  131 x 122 = 16492   the 160 KiB ones (1024 threads), every env in LDS
  182 x 176 = 32752   the 160 KiB ones, every env in LDS
  183 x 176 = 32930   the 160 KiB ones, the boundary env in global memory and its small neighbours in LDS
each once single-goal and twice seeded (a call has one `where` and one `among`: the two kinds of seed set are two launches)."""
import time

import numpy as np
import pytest
import torch

from tests.test_navfield_host import CELL, F, INF, bits, nav_rule
from tests.test_navseed_host import seed_rule
from tests.test_gpu_navseen import _by_hand, _np

pytestmark = pytest.mark.gpu

# (which capacity, columns, rows, framed cells): written out, not derived from the constant - a change of capacity fails the
# assertion in _World instead of moving the test off the boundary
SHAPES = [(0, 110, 71, 8176), (0, 111, 71, 8249), (1, 130, 122, 16368), (1, 131, 122, 16492), (2, 182, 176, 32752), (2, 183, 176, 32930)]
BOUNDARY, SMALL, TALL, WIDE, SINGLE, BLOCKED, NONE = range(7)
N_POINTS = 32
SENTINEL = -7.25


def _centre(geom, i, j):
    x, y = nav_rule.centres(geom, CELL)
    return np.array([x[j], y[i]], F)


def _middle_free(free):
    """The free cell nearest the middle of the env."""
    i, j = np.nonzero(free)
    k = np.argmin((i - free.shape[0]//2)**2 + (j - free.shape[1]//2)**2)
    return int(i[k]), int(j[k])


class _World:
    """One launch's envs, laid out by hand on the host, with the rule's graphs; the device grid is made on first use."""

    def __init__(self, which, nx, ny, framed):
        from megastep_amd import cuda
        assert (nx + 2)*(ny + 2) == framed
        at_capacity = framed == cuda.FIELD_CAPACITY[which]
        assert at_capacity or cuda.FIELD_CAPACITY[which] < framed <= cuda.FIELD_CAPACITY[which] + ny + 2      # (one column more)
        self.which, self.at_capacity, self.framed = which, at_capacity, framed
        # the tier the host picks for the launch, and whether the boundary env relaxes in LDS there
        self.tier = which if at_capacity else min(which + 1, 2)
        self.in_lds = framed <= cuda.FIELD_CAPACITY[self.tier]
        assert self.in_lds == (at_capacity or which < 2)
        rng = np.random.RandomState(100 + framed)
        big = rng.rand(ny, nx) < .8
        big[ny - 2:, nx - 1] = True                                     # (the two anchors of the goal in the last row and column)
        self.envs = [((-37, -52, nx, ny), big), ((3, -4, 9, 7), rng.rand(7, 9) < .8), ((-2, 5, 1, 300), rng.rand(300, 1) < .97),
                     ((-150, -1, 300, 1), rng.rand(1, 300) < .97), ((4, 4, 1, 1), np.ones((1, 1), bool)),
                     ((0, 0, 5, 5), np.zeros((5, 5), bool)), ((0, 0, 0, 0), np.zeros((0, 0), bool))]
        self.n = len(self.envs)
        self.graphs = [nav_rule._neighbours(free, CELL) if free.size else None for _, free in self.envs]
        self._grid = None

    @property
    def grid(self):
        if self._grid is None:
            self._grid = _by_hand(self.envs)
            assert self._grid._max_framed == self.framed
        return self._grid

    def goals(self):
        """(N, 2, 2) float32. The boundary env: one a few centimetres off the centre of the free cell nearest the middle, one in
        the last row and column, right of and below that cell's centre - two of its four anchors lie outside the grid."""
        goals, rng = np.zeros((self.n, 2, 2), F), np.random.RandomState(200 + self.framed)
        for e, (geom, free) in enumerate(self.envs):
            jx0, iy0, nx, ny = geom
            if not free.size:
                goals[e] = [[1., 1.], [np.nan, 0.]]
                continue
            lo, hi = np.array([jx0, iy0])*CELL, np.array([jx0 + nx, iy0 + ny])*CELL
            goals[e] = (lo + rng.uniform(0, 1, (2, 2))*(hi - lo)).astype(F)
        geom, free = self.envs[BOUNDARY]
        goals[BOUNDARY, 0] = _centre(geom, *_middle_free(free)) + np.array([.03, -.02], F)
        goals[BOUNDARY, 1] = _centre(geom, geom[3] - 1, geom[2] - 1) + np.array([.03, -.02], F)
        assert len(nav_rule.anchors(goals[BOUNDARY, 1], geom, CELL, free)) == 2
        for e in (TALL, WIDE):
            geom, free = self.envs[e]
            goals[e, 0] = _centre(geom, *_middle_free(free)) + np.array([.01, .02], F)
        goals[SINGLE, 0] = _centre(self.envs[SINGLE][0], 0, 0)         # on its cell's centre: the field is +0
        goals[SINGLE, 1] = _centre(self.envs[SINGLE][0], 0, 0) + np.array([-.04, .05], F)
        goals[BLOCKED] = _centre(self.envs[BLOCKED][0], 2, 2) + np.array([[.01, .01], [-.2, .1]], F)
        return goals

    def points(self):
        """(N, N_POINTS, 2) float32 and the field each asks: spread over the env and half a cell round it, on the outer ring from
        outside (one or two anchors), not numbers, far away; a few field indices that name no field."""
        pts, rng = np.zeros((self.n, N_POINTS, 2), F), np.random.RandomState(300 + self.framed)
        for e, (geom, free) in enumerate(self.envs):
            jx0, iy0, nx, ny = geom
            lo, hi = (np.array([jx0, iy0]) - .5)*CELL, (np.array([jx0 + nx, iy0 + ny]) + .5)*CELL
            pts[e] = (lo + rng.uniform(0, 1, (N_POINTS, 2))*(hi - lo)).astype(F)
            if free.size:
                x, y = nav_rule.centres(geom, CELL)
                pts[e, 0] = [x[0] - .03, y[0] - .04]                    # one anchor: the corner cells
                pts[e, 1] = [x[-1] + .03, y[-1] + .04]
                pts[e, 2] = [x[0] - .03, y[ny//2] + .01]                # two: the first and the last column, the first and the last row
                pts[e, 3] = [x[-1] + .05, y[ny//2] - .01]
                pts[e, 4] = [x[nx//2] + .02, y[0] - .05]
                pts[e, 5] = [x[nx//2] - .02, y[-1] + .03]
            pts[e, 6] = [np.nan, pts[e, 6, 1]]
            pts[e, 7] = [np.nan, np.nan]
            pts[e, 8] = [pts[e, 8, 0], np.inf]
            pts[e, 9] = [1e6, -1e6]
        which = rng.randint(0, 2, (self.n, N_POINTS)).astype(np.int32)
        which[:, 10] = 2
        which[:, 11] = -1
        return pts, which


_WORLDS = {}


def _world(shape):
    if shape not in _WORLDS:
        _WORLDS[shape] = _World(*shape)
    return _WORLDS[shape]


def _worth(field, free, distinct=1000):
    """The conditions that keep an equality on the boundary env from being an empty one: finite on more than half of the free
    cells, more than 1000 distinct values. (A seeded field of 1 % seeds cannot hold that many: a cell is some five cells from
    its nearest seed, and a value is a straight steps and b diagonal ones with a + b below 30 or so - a few hundred sums; the
    seeded tests ask for more than 100.)"""
    return int(np.isfinite(field).sum()) > free.sum()/2 and len(np.unique(field[np.isfinite(field)])) > distinct


def _ids(shape):
    return f'{shape[1]}x{shape[2]}'


@pytest.mark.parametrize('shape', SHAPES, ids=_ids)
def test_single_goal_fields_and_queries_are_the_rules_bits_at_the_capacity_and_a_column_beyond(shape):
    from megastep_amd import cuda
    began = time.time()
    w = _world(shape)
    grid, goals = w.grid, w.goals()
    want = [[nav_rule.field(free, geom, CELL, goals[e, g], w.graphs[e]) if free.size else np.zeros((0, 0), F) for g in range(2)]
            for e, (geom, free) in enumerate(w.envs)]
    for g in range(2):
        assert _worth(want[BOUNDARY][g], w.envs[BOUNDARY][1]), g
    fields = cuda.distance_fields(grid, torch.as_tensor(goals, device='cuda'), passes=True)
    for e in range(w.n):
        for g in range(2):
            got = _np(fields.image(e, g))
            assert np.array_equal(bits(got), bits(want[e][g])), (e, g, int((bits(got) != bits(want[e][g])).sum()))
    passes = _np(fields.passes)
    print(f'single-goal, {_ids(shape)} = {w.framed} framed cells, tier {w.tier}, the boundary env in {"LDS" if w.in_lds else "global memory"}: '
          f'passes {passes.reshape(-1).tolist()}')
    assert (passes[:NONE] >= 1).all() and (passes[[SINGLE, BLOCKED]] == 1).all() and (passes[NONE] == 0).all()
    assert np.isinf(want[BLOCKED][0]).all() and bits(want[SINGLE][0]).tolist() == [[0]] and np.isfinite(want[TALL][0]).sum() > 5
    # the query
    pts, which = w.points()
    got_q = _np(fields.at(torch.as_tensor(pts, device='cuda'), goal=torch.as_tensor(which, device='cuda')))
    want_q = np.full(which.shape, INF, F)
    for e, (geom, free) in enumerate(w.envs):
        for k in range(N_POINTS):
            if free.size and 0 <= which[e, k] < 2:
                want_q[e, k] = nav_rule.query(want[e][which[e, k]], geom, CELL, free, pts[e, k])
    assert np.array_equal(bits(got_q), bits(want_q)), np.argwhere(bits(got_q) != bits(want_q)).tolist()
    assert np.isinf(want_q[:, 6:12]).all() and np.isinf(want_q[NONE]).all() and np.isfinite(want_q[BOUNDARY]).sum() >= 10
    assert np.isfinite(want_q[:BLOCKED, :6]).sum() >= 12                # (the ring's points: most find their one or two anchors free)
    # mask and out on sentinel-filled values: a masked-out field keeps every bit and reports no pass
    fields.values.fill_(SENTINEL)
    fields.passes.zero_()
    mask = np.ones((w.n, 2), bool)
    mask[[BOUNDARY, SMALL, TALL, SINGLE], [1, 0, 1, 0]] = False
    mask[WIDE] = False
    same = cuda.distance_fields(grid, torch.as_tensor(goals, device='cuda'), mask=torch.as_tensor(mask, device='cuda'), out=fields)
    assert same is fields
    again = _np(fields.passes)
    for e in range(w.n):
        for g in range(2):
            got = _np(fields.image(e, g))
            kept = np.full(got.shape, SENTINEL, F)
            assert np.array_equal(bits(got), bits(want[e][g] if mask[e, g] else kept)), (e, g)
    assert (again[~mask] == 0).all() and (again[:NONE][mask[:NONE]] >= 1).all() and (again[NONE] == 0).all()
    print(f'  with the mask: passes {again.reshape(-1).tolist()}; {time.time() - began:.2f} s')


def _bytes(rng, bit0):
    """Bytes whose bit 0 is `bit0` and whose bit 1 is drawn: values in {0, 1, 2, 3}, of which only bit 0 may count."""
    return (bit0.astype(np.uint8) | (rng.randint(0, 2, bit0.shape) << 1)).astype(np.uint8)


def _seed_sets(w, where):
    """(marks in the fields' layout, among in the grid's layout or None, [env][field] (ny, nx) bool seeds by seed_rule).
    where=True: the seeds are the marked cells, 1 % of them on the boundary env, without an `among` layer; where=False: the
    unmarked cells among a layer of half the cells. The small envs carry the degenerate sets: no seed at all, every free cell a
    seed."""
    rng = np.random.RandomState(7 + w.framed + where)
    marks, among, seeds = [], [], []
    for e, (geom, free) in enumerate(w.envs):
        share = [(.01, .01), (.1, .3), (.01, 1.), (.01, .05), (1., 0.), (1., .5), (0., 0.)][e]
        layer = rng.rand(*free.shape) < .5
        if e == SMALL:
            share, layer = ((.1, 0.) if where else (.2, 1.)), np.ones(free.shape, bool)    # field 1: no seed at all / every free cell
        if e == TALL and not where:
            layer[:] = False                                            # among nobody: no seed, whatever the marks
        among.append(_bytes(rng, layer).reshape(-1))
        row = []
        for g in range(2):
            chosen = rng.rand(*free.shape) < share[g]
            if e in (TALL, WIDE) and g == 0 and free.size:
                chosen[_middle_free(free)] = True
            m = _bytes(rng, chosen if where else ~chosen)
            marks.append(m.reshape(-1))
            row.append(seed_rule.seeds(free, m, where, None if where else among[-1].reshape(free.shape)))
        seeds.append(row)
    return np.concatenate(marks + [np.zeros(0, np.uint8)]), None if where else np.concatenate(among + [np.zeros(1, np.uint8)]), seeds


@pytest.mark.parametrize('where', [True, False])
@pytest.mark.parametrize('shape', SHAPES, ids=_ids)
def test_seeded_fields_are_the_rules_bits_at_the_capacity_and_a_column_beyond(shape, where):
    from megastep_amd import cuda
    began = time.time()
    w = _world(shape)
    grid = w.grid
    marks, among, seeds = _seed_sets(w, where)
    assert marks.max() == 3 and marks.shape[0] == 2*grid.n_cells
    want = [[seed_rule.field(free, CELL, seeds[e][g], w.graphs[e]) if free.size else np.zeros((0, 0), F) for g in range(2)]
            for e, (_, free) in enumerate(w.envs)]
    counts = np.array([[s.sum() for s in row] for row in seeds], np.int32)
    for g in range(2):
        assert _worth(want[BOUNDARY][g], w.envs[BOUNDARY][1], 100) and 0 < counts[BOUNDARY, g] < w.envs[BOUNDARY][1].sum()/20, g
    got = cuda.seeded_fields(grid, torch.as_tensor(marks, device='cuda'), 2, where=where,
                             among=None if among is None else torch.as_tensor(among, device='cuda'), passes=True)
    assert np.array_equal(_np(got.n_seeds), counts), (_np(got.n_seeds).tolist(), counts.tolist())
    for e in range(w.n):
        for g in range(2):
            have = _np(got.image(e, g))
            assert np.array_equal(bits(have), bits(want[e][g])), (e, g, int((bits(have) != bits(want[e][g])).sum()))
    passes = _np(got.passes)
    print(f'seeded, where={where}, {_ids(shape)} = {w.framed} framed cells, tier {w.tier}, the boundary env in '
          f'{"LDS" if w.in_lds else "global memory"}: seeds {counts.reshape(-1).tolist()}, passes {passes.reshape(-1).tolist()}; '
          f'{time.time() - began:.2f} s')
    # nothing can be lowered where there is no seed, and where every free cell is one
    settled = np.array([[not s.any() or np.array_equal(s, free) for s in row] for row, (_, free) in zip(seeds, w.envs)])
    assert (passes[:NONE] >= 1).all() and (passes[:NONE][settled[:NONE]] == 1).all() and (passes[NONE] == 0).all()
    assert (passes[BOUNDARY] >= 2).all() and (counts[[BLOCKED, NONE]] == 0).all() and np.isinf(want[BLOCKED][0]).all()
    none, every = (SMALL, 1) if where else (TALL, 1), (TALL, 1) if where else (SMALL, 1)
    assert counts[none] == 0 and np.isinf(want[none[0]][none[1]]).all() and w.envs[none[0]][1].any()
    free = w.envs[every[0]][1]
    assert counts[every] == free.sum() > 0 and (want[every[0]][every[1]][free] == 0).all()
