"""Cell draws (`ms_nav_draws`, `cuda.cell_draws`) on the CPU: the contract of include/megastep_hip.h (MsNavDraws) restated in
numpy (`draw_rule`, which tests/test_gpu_navdraw.py holds the kernel to, exactly); the host instantiation of the kernel's own
device functions against the rule, on hand-made grids chosen where a bitmap, a scan and a select can go wrong, and on real
plans; the hash's known answers; the mask and the counter; the uniformity of the draws as chi-square conditions; and the
C-ABI's declarations, layouts and refusals."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests.test_abi import ROOT, declared_symbols
from tests.test_navfield_host import CELL, CELLS, RADIUS, F, bits, nav_rule
from tests.test_navwindow_host import Layer

INF, NAN = F(np.inf), F(np.nan)
U = np.uint32


class draw_rule:
    """The contract in numpy: 32-bit integer arithmetic modulo 2^32, one 64-bit product for the rank."""

    @staticmethod
    def mix(a):
        a = np.asarray(a, U).copy()
        a ^= a >> U(16)
        a *= U(0x85ebca6b)
        a ^= a >> U(13)
        a *= U(0xc2b2ae35)
        a ^= a >> U(16)
        return a

    @staticmethod
    def hash(seed, which, counter, k, stream):
        """h = fold(seed_lo, seed_hi, n*P + p, counter, k, stream), broadcasting over arrays."""
        words = (seed & 0xffffffff, seed >> 32, which, counter, k, stream)
        s = U(0x9e3779b9)
        for word in words:
            s = draw_rule.mix(np.asarray(s, U) + (np.asarray(word, np.int64) & 0xffffffff).astype(U))
        return s

    @staticmethod
    def rank(h, M):
        return ((np.asarray(h, np.uint64)*np.uint64(M)) >> np.uint64(32)).astype(np.int64)

    @staticmethod
    def uniform(h):
        return (np.asarray(h, U) >> U(8)).astype(F)*F(2.**-24)

    @staticmethod
    def store(layer, n, p):
        f = int(layer.field[n, p]) if layer.field is not None else (0 if layer.n_fields == 1 else p)
        return f if 0 <= f < layer.n_fields else -1

    @staticmethod
    def qualifying(free, source, first, n_cells, n, p, where=True, lo=None, hi=None, gate=None):
        """(the env's qualifying cells in row-major order, the store's values or None): set (n, p) of an env of n_cells from `first`."""
        fs = draw_rule.store(source, n, p)
        fg = draw_rule.store(gate, n, p) if gate is not None else 0
        if n_cells == 0 or fs < 0 or fg < 0:
            return np.zeros(0, np.int64), None
        values = source.values[source.n_fields*first + fs*n_cells:][:n_cells]
        ok = free[first:first + n_cells] != 0
        if source.is_float:
            with np.errstate(invalid='ignore'):
                ok &= (F(lo) <= values) & (values <= F(hi))
        else:
            ok &= (values != 0) == bool(where)
        if gate is not None:
            ok &= gate.values[gate.n_fields*first + fg*n_cells:][:n_cells] != 0
        return np.flatnonzero(ok), values

    @staticmethod
    def call(geom, starts, cell, free, source, P, K, counter, lo=None, hi=None, where=True, gate=None, seed=0, mask=None, before=None):
        """One call of ms_nav_draws: dict(cells, points, uniforms, values, counts, counter); `before`: what the outputs held (for the
        sets the mask leaves out; required with one)."""
        N = len(geom)
        if before is None:
            assert mask is None
            before = dict(cells=np.empty((N, P, K), np.int32), points=np.empty((N, P, K, 2), F), uniforms=np.empty((N, P, K), F),
                          values=np.empty((N, P, K), F) if source.is_float else None, counts=np.empty((N, P), np.int32))
        out = {k: None if v is None else v.copy() for k, v in before.items()}
        out['counter'] = np.array(counter, np.int32)
        ks = np.arange(K)
        for n in range(N):
            jx0, iy0, nx, ny = (int(v) for v in geom[n])
            n_cells = nx*ny if nx > 0 and ny > 0 else 0
            for p in range(P):
                if mask is not None and not mask[n, p]:
                    continue
                q, values = draw_rule.qualifying(free, source, int(starts[n]), n_cells, n, p, where, lo, hi, gate)
                M, count = len(q), int(out['counter'][n, p])
                out['uniforms'][n, p] = draw_rule.uniform(draw_rule.hash(seed, n*P + p, count, ks, 1))
                if M:
                    chosen = q[draw_rule.rank(draw_rule.hash(seed, n*P + p, count, ks, 0), M)]
                    i, j = chosen//nx, chosen % nx
                    out['cells'][n, p] = chosen
                    out['points'][n, p, :, 0] = ((jx0 + j).astype(F) + F(.5))*F(cell)
                    out['points'][n, p, :, 1] = ((iy0 + i).astype(F) + F(.5))*F(cell)
                    if source.is_float:
                        out['values'][n, p] = values[chosen]
                else:
                    out['cells'][n, p], out['points'][n, p] = -1, NAN
                    if source.is_float:
                        out['values'][n, p] = NAN
                out['counts'][n, p] = M
                out['counter'][n, p] = (count + 1 + 2**31) % 2**32 - 2**31              # (modulo 2^32, as an int32)
        return out


def _aligned(geom):
    geom = np.ascontiguousarray(geom, np.int32)
    if geom.ctypes.data % 16:                        # (MsNavGrid.geom: 16-byte aligned)
        room = np.empty(geom.size + 4, np.int32)
        off = (-room.ctypes.data % 16)//4
        room[off:off + geom.size] = geom.reshape(-1)
        geom = room[off:off + geom.size].reshape(geom.shape)
    return geom


def _layer_spec(layer, keep):
    from megastep_amd import _lib
    keep += [layer.values, layer.field]
    return _lib.MsNavLayer(layer.values.ctypes.data, int(layer.is_float), layer.n_fields, None if layer.field is None else layer.field.ctypes.data)


class _Host:
    """ms_host_nav_draws on host arrays, the outputs its own (sentinels to begin with): call after call moves the counter on."""

    def __init__(self, geom, starts, cell, free, source, P, K, counter=None, lo=None, hi=None, where=True, gate=None, seed=0, clearance=RADIUS):
        from megastep_amd import _lib
        self.geom, self.starts, self.free = _aligned(geom), np.ascontiguousarray(starts, np.int64), np.ascontiguousarray(free, np.uint8)
        N = len(self.geom)
        self.out = dict(cells=np.full((N, P, K), -7, np.int32), points=np.full((N, P, K, 2), F(-7), F), uniforms=np.full((N, P, K), F(-7), F),
                        values=np.full((N, P, K), F(-7), F) if source.is_float else None, counts=np.full((N, P), -7, np.int32))
        self.counter = np.zeros((N, P), np.int32) if counter is None else np.array(counter, np.int32)
        self._keep = []
        cells = self.geom[:, 2].astype(np.int64)*self.geom[:, 3]
        self.grid = _lib.MsNavGrid(N, cell, clearance, self.geom.ctypes.data, self.starts.ctypes.data, 0, self.free.ctypes.data)
        o = self.out
        self.spec = _lib.MsNavDraws(source=_layer_spec(source, self._keep), gate=_layer_spec(gate, self._keep) if gate is not None else _lib.MsNavLayer(),
                                    where=int(bool(where)), lo=0. if lo is None else float(lo), hi=0. if hi is None else float(hi), n_sets=P, n_draws=K,
                                    seed=seed, counter=self.counter.ctypes.data, mask=None, cells=o['cells'].ctypes.data,
                                    points=o['points'].ctypes.data, uniforms=o['uniforms'].ctypes.data,
                                    values=None if o['values'] is None else o['values'].ctypes.data, counts=o['counts'].ctypes.data,
                                    max_cells=int(max(cells.max(initial=0), 0)))
        self._call = _lib.lib().ms_host_nav_draws

    def __call__(self, mask=None):
        mask = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        self.spec.mask = None if mask is None else mask.ctypes.data
        assert self._call(ctypes.byref(self.grid), ctypes.byref(self.spec)) == 0
        return dict(self.out, counter=self.counter)


def same(got, want):
    """Are two results of a call equal - floats as bits, NaN included?"""
    for key in ('cells', 'counts', 'counter'):
        assert np.array_equal(got[key], want[key]), (key, int((np.asarray(got[key]) != np.asarray(want[key])).sum()))
    for key in ('points', 'uniforms', 'values'):
        assert (got[key] is None) == (want[key] is None), key
        if want[key] is not None:
            assert np.array_equal(bits(got[key]), bits(want[key])), (key, int((bits(got[key]) != bits(want[key])).sum()))


def _same(geom, starts, free, source, P, K, counter=None, cell=CELL, clearance=RADIUS, **kw):
    """One call of the host instantiation against one of the rule; returns the rule's result."""
    host = _Host(geom, starts, cell, free, source, P, K, counter=counter, clearance=clearance, **kw)
    counter = host.counter.copy()
    want = draw_rule.call(geom, starts, cell, free, source, P, K, counter, **kw)
    same(host(), want)
    return want


# ---------------------------------------------------------------------------------------------------------------------
# the hash
# ---------------------------------------------------------------------------------------------------------------------
def test_the_hash_has_its_known_answers_and_the_uniform_is_its_top_24_bits():
    assert int(draw_rule.hash(0, 0, 0, 0, 0)) == 0xe88cf1a4
    assert int(draw_rule.hash(12345, 2, 9, 4, 0)) == 0xf8f4d17a
    # through the host instantiation: a grid of 2^16 cells, all qualifying, M = 2^16: the rank is h's top 16 bits
    geom, starts, free = np.array([[0, 0, 256, 256]], np.int32), np.array([0, 65536], np.int64), np.ones(65536, np.uint8)
    got = _Host(geom, starts, CELL, free, Layer(free), 1, 1)()
    assert int(got['cells'][0, 0, 0]) == 0xe88cf1a4 >> 16 and int(got['counts'][0, 0]) == 65536
    host = _Host(geom, starts, CELL, free, Layer(free), 3, 5, counter=np.full((1, 3), 9), seed=12345)
    got = host()
    assert int(got['cells'][0, 2, 4]) == 0xf8f4d17a >> 16
    k = np.arange(5)
    for p in range(3):
        h1 = draw_rule.hash(12345, p, 9, k, 1)
        assert np.array_equal(bits(got['uniforms'][0, p]), bits((h1 >> U(8)).astype(np.float64)*2.**-24))
    assert (got['uniforms'] >= 0).all() and (got['uniforms'] < 1).all()
    assert float(draw_rule.uniform(U(0xffffffff))) == 1 - 2.**-24 and float(draw_rule.uniform(U(0xff))) == 0.


# ---------------------------------------------------------------------------------------------------------------------
# hand-made grids
# ---------------------------------------------------------------------------------------------------------------------
class _Hand:
    pass


_HAND = []


def hand():
    """One grid of nine envs: 1 x 1; 3 x 5; 65 cells; 64*256 + 1 cells; only the last cell free; none free; all free; no cells;
    and 64 cells.  Envs 0 to 3 and 8 have random free cells (most of them free)."""
    if not _HAND:
        w = _Hand()
        rng = np.random.RandomState(5)
        w.geom = np.array([(0, 0, 1, 1), (-2, 3, 3, 5), (7, -9, 65, 1), (-50, -60, 113, 145), (1, 1, 10, 7), (1, 1, 10, 7), (-4, 0, 9, 9),
                           (3, 4, 0, 7), (0, 0, 8, 8)], np.int32)
        sizes = np.maximum(w.geom[:, 2].astype(np.int64)*w.geom[:, 3], 0)
        assert sizes.tolist() == [1, 15, 65, 64*256 + 1, 70, 70, 81, 0, 64]
        w.starts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        w.n_cells = int(w.starts[-1])
        free = (rng.uniform(size=w.n_cells) < .8).astype(np.uint8)
        free[w.starts[0]] = 1
        free[w.starts[3]], free[w.starts[4] - 1] = 1, 1                   # (the first and the last cell of the large env)
        free[w.starts[4]:w.starts[5]] = 0
        free[w.starts[5] - 1] = 3                                        # (any non-zero byte is free)
        free[w.starts[5]:w.starts[6]] = 0
        free[w.starts[6]:w.starts[7]] = 1
        w.free = free
        w.N = len(w.geom)
        _HAND.append(w)
    return _HAND[0]


@pytest.mark.parametrize('K', [1, 7, 256])
def test_free_cells_alone_on_the_hand_made_grids(K):
    w = hand()
    want = _same(w.geom, w.starts, w.free, Layer(w.free), 2, K, seed=K)
    sizes = np.diff(w.starts)
    assert want['counts'][:, 0].tolist() == [int(w.free[w.starts[e]:w.starts[e + 1]].astype(bool).sum()) for e in range(w.N)]
    assert want['counts'][[4, 5, 6, 7], 1].tolist() == [1, 0, 81, 0]
    assert (want['cells'][4] == 69).all() and (want['cells'][[5, 7]] == -1).all() and np.isnan(want['points'][[5, 7]]).all()
    assert (want['cells'][0] == 0).all() and np.array_equal(want['points'][0, 0, 0], [F(.5)*F(CELL)]*2)
    assert ((want['cells'] >= -1) & (want['cells'] < sizes[:, None, None])).all()
    if K == 256:
        assert (want['cells'][3] > 64*255).any() and (want['cells'][3] < 64).any()           # (the first and the last lane's span)
        assert len(np.unique(want['cells'][6])) > 60 and not np.array_equal(want['cells'][6, 0], want['cells'][6, 1])
    # the centre of the last cell of the 3 x 5 env, by hand: column 2, row 4 of a grid from (-2, 3)
    at = np.argwhere(want['cells'][1] == 14)
    if len(at):
        assert np.array_equal(want['points'][1][tuple(at[0])], [F(.5)*F(CELL), F(7.5)*F(CELL)])


@pytest.mark.parametrize('K', [1, 7, 256])
@pytest.mark.parametrize('gated', [False, True])
@pytest.mark.parametrize('where', [True, False])
def test_byte_sources_in_both_senses_with_and_without_a_gate(K, gated, where):
    w = hand()
    rng = np.random.RandomState(11 + K)
    marks = rng.choice(np.array([0, 0, 1, 2, 255], np.uint8), 3*w.n_cells)
    gate = Layer(rng.choice(np.array([0, 1, 7], np.uint8), w.n_cells)) if gated else None
    want = _same(w.geom, w.starts, w.free, Layer(marks, 3), 3, K, where=where, gate=gate, seed=2**40 + 7, counter=rng.randint(0, 1000, (w.N, 3)))
    assert (want['counts'][[1, 2, 3, 6, 8]] > 0).all() and (want['counts'][[5, 7]] == 0).all()
    for n, p in ((3, 0), (3, 2), (6, 1)):
        first, n_cells = int(w.starts[n]), int(w.starts[n + 1] - w.starts[n])
        cells = want['cells'][n, p]
        assert (w.free[first + cells] != 0).all() and ((marks[3*first + p*n_cells + cells] != 0) == where).all()
        assert not gated or (gate.values[first + cells] != 0).all()


@pytest.mark.parametrize('K', [1, 7, 256])
def test_a_float_band_takes_both_its_ends_and_neither_a_nan_nor_an_infinity(K):
    w = hand()
    rng = np.random.RandomState(17)
    lo, hi = F(1.1), F(2.7)
    D = rng.uniform(0., 4., 2*w.n_cells).astype(F)
    D[::7], D[1::7], D[2::7], D[3::11], D[5::13] = lo, hi, NAN, INF, -INF
    D[4::7], D[6::7] = np.nextafter(lo, F(0)), np.nextafter(hi, F(9))             # (just outside)
    want = _same(w.geom, w.starts, w.free, Layer(D, 2), 2, K, lo=lo, hi=hi, seed=3)
    got = want['values'][want['cells'] >= 0]
    assert ((got >= lo) & (got <= hi)).all() and (K < 7 or ((got == lo).any() and (got == hi).any()))
    assert np.isnan(want['values'][want['cells'] < 0]).all()
    # an infinite band takes the infinities, never the NaN; an empty band takes nothing
    every = _same(w.geom, w.starts, w.free, Layer(D, 2), 2, K, lo=-INF, hi=INF)
    assert not np.isnan(every['values'][every['cells'] >= 0]).any() and (K < 256 or np.isinf(every['values']).any())
    none = _same(w.geom, w.starts, w.free, Layer(D, 2), 2, K, lo=hi, hi=lo)
    assert (none['counts'] == 0).all() and (none['cells'] == -1).all()
    gated = _same(w.geom, w.starts, w.free, Layer(D[:w.n_cells]), 4, K, lo=lo, hi=hi, gate=Layer(rng.randint(0, 2, 4*w.n_cells).astype(np.uint8), 4))
    assert (gated['counts'][3] > 100).all() and len(set(gated['counts'][3].tolist())) > 1


def test_a_field_names_the_store_each_set_reads_and_a_bad_index_leaves_it_empty():
    w = hand()
    rng = np.random.RandomState(23)
    marks = rng.randint(0, 2, 3*w.n_cells).astype(np.uint8)
    D = rng.uniform(0., 4., 2*w.n_cells).astype(F)
    field = rng.randint(0, 3, (w.N, 4))
    field[3], field[6] = [2, 2, 0, 1], [0, 3, -1, 1]                          # (3 and -1: no store of three)
    gate_field = rng.randint(0, 3, (w.N, 4))
    gate_field[8] = [0, 5, 1, 2]
    want = _same(w.geom, w.starts, w.free, Layer(marks, 3, field), 4, 7)
    assert want['counts'][6].tolist()[1:3] == [0, 0] and (want['counts'][6, [0, 3]] > 0).all() and want['counts'][3, 0] == want['counts'][3, 1]
    assert (want['cells'][6, 1:3] == -1).all() and np.array_equal(want['counter'], np.ones((w.N, 4), np.int32))
    want = _same(w.geom, w.starts, w.free, Layer(D, 2, field % 2), 4, 7, lo=1., hi=3., gate=Layer(marks, 3, gate_field))
    assert want['counts'][8, 1] == 0 and (want['counts'][8, [0, 2, 3]] > 0).all() and np.isnan(want['values'][8, 1]).all()
    # n_fields of 1 and of P without a field: one store, one per set
    one = _same(w.geom, w.starts, w.free, Layer(marks[:w.n_cells]), 3, 7)
    per = _same(w.geom, w.starts, w.free, Layer(marks, 3), 3, 7)
    assert (one['counts'][3] == one['counts'][3, 0]).all() and len(set(per['counts'][3].tolist())) == 3


# ---------------------------------------------------------------------------------------------------------------------
# real plans
# ---------------------------------------------------------------------------------------------------------------------
_PLANS = {}


def plan_world(cell=CELL, r=RADIUS):
    """test_navseen_host's six plans (three plain, three oblique) as ONE grid, and the rule's distance field round each plan's
    first viewer: (geom, starts, free, D)."""
    if (cell, r) not in _PLANS:
        from tests.test_navseen_host import cases
        cs = cases(cell, r)
        geom = np.array([c.geom for c in cs], np.int32)
        starts = np.concatenate([[0], np.cumsum([c.free.size for c in cs])]).astype(np.int64)
        free = np.concatenate([c.free.reshape(-1).astype(np.uint8) for c in cs])
        D = np.concatenate([nav_rule.field(c.free, c.geom, cell, c.origins[0]).reshape(-1) for c in cs])
        _PLANS[cell, r] = (geom, starts, free, D)
    return _PLANS[cell, r]


def test_on_real_plans_every_drawn_cell_is_free_and_at_a_distance_in_the_band():
    _drawn_cells_are_free_and_in_the_band(CELL, RADIUS)


@pytest.mark.parametrize('cell,r', CELLS)
def test_on_real_plans_the_draws_are_the_rule_at_other_cell_widths(cell, r):
    """A drawn point is its cell's centre, ((origin + k) + .5)*c: rounded when the cell is no power of two."""
    _drawn_cells_are_free_and_in_the_band(cell, r)


def _drawn_cells_are_free_and_in_the_band(cell, r):
    geom, starts, free, D = plan_world(cell, r)
    lo, hi = F(2.), F(5.)
    for K in (1, 7, 256):
        want = _same(geom, starts, free, Layer(D), 2, K, lo=lo, hi=hi, seed=K, cell=cell, clearance=r)
        assert (want['counts'] > 50).all() and (want['cells'] >= 0).all()
        at = starts[:-1, None, None] + want['cells']
        assert (free[at] != 0).all() and np.array_equal(bits(D[at]), bits(want['values']))
        assert ((want['values'] >= lo) & (want['values'] <= hi)).all()
        for n in range(len(geom)):
            x, y = nav_rule.centres(tuple(geom[n]), cell)
            nx = int(geom[n, 2])
            assert np.array_equal(want['points'][n, ..., 0], x[want['cells'][n] % nx]) and np.array_equal(want['points'][n, ..., 1], y[want['cells'][n]//nx])
    assert len(np.unique(want['cells'][0])) > 100


# ---------------------------------------------------------------------------------------------------------------------
# the mask and the counter
# ---------------------------------------------------------------------------------------------------------------------
def test_a_masked_out_set_is_not_touched_and_a_computed_one_counts_one_call():
    w = hand()
    rng = np.random.RandomState(29)
    D = rng.uniform(0., 4., w.n_cells).astype(F)
    source = Layer(D)
    start = rng.randint(0, 100, (w.N, 3)).astype(np.int32)
    start[2, 1] = 2**31 - 1                                               # (the counter wraps as 32 bits do)
    host = _Host(w.geom, w.starts, CELL, w.free, source, 3, 7, counter=start, lo=1., hi=3., seed=99)
    mask = rng.uniform(size=(w.N, 3)) < .5
    mask[2, 1], mask[3, 0], mask[3, 1] = True, True, False
    blank = {k: None if v is None else v.copy() for k, v in host.out.items()}
    got = {k: v.copy() for k, v in host(mask).items()}
    want = draw_rule.call(w.geom, w.starts, CELL, w.free, source, 3, 7, start, lo=1., hi=3., seed=99, mask=mask, before=blank)
    same(got, want)
    assert np.array_equal(got['counter'].astype(np.int64), (start.astype(np.int64) + mask + 2**31) % 2**32 - 2**31) and got['counter'][2, 1] == -2**31
    assert (got['cells'][~mask] == -7).all() and (got['counts'][~mask] == -7).all() and (got['uniforms'][~mask] == -7).all()
    assert (got['values'][~mask] == -7).all() and (got['points'][~mask] == -7).all() and (got['counts'][mask][:3] >= 0).all()
    # two calls in a row: the rule at counter and at counter + 1
    host = _Host(w.geom, w.starts, CELL, w.free, source, 3, 7, counter=start, lo=1., hi=3., seed=99)
    first = {k: None if v is None else v.copy() for k, v in host().items()}
    second = host()
    want1 = draw_rule.call(w.geom, w.starts, CELL, w.free, source, 3, 7, start, lo=1., hi=3., seed=99)
    want2 = draw_rule.call(w.geom, w.starts, CELL, w.free, source, 3, 7, want1['counter'], lo=1., hi=3., seed=99)
    same(first, want1)
    same(second, want2)
    assert not np.array_equal(first['cells'][3], second['cells'][3]) and np.array_equal(first['counts'], second['counts'])


# ---------------------------------------------------------------------------------------------------------------------
# uniformity: conditions on chi-square statistics at their 0.001 points, which the rule's own hash meets (worst values over
# the four seeds: 74.0 for M = 64, 45.1 for 37, 1067.3 for 1000, 72.9 and 62.6 for the two joint tables)
# ---------------------------------------------------------------------------------------------------------------------
def _chi2(counts, total):
    expected = total/counts.size
    return float(((counts - expected)**2/expected).sum())


def _strip(M):
    """A one-row env of M + 3 cells of which M are free: the r-th qualifying cell is not cell r."""
    free = np.ones(M + 3, np.uint8)
    free[[0, M//2, M + 1]] = 0
    return np.array([[0, 0, M + 3, 1]], np.int32), np.array([0, M + 3], np.int64), free


DRAWS = 64000


@pytest.mark.parametrize('seed', [0, 1, 12345, 2**40 + 7])
@pytest.mark.parametrize('M, limit', [(64, 103.4), (37, 68.0), (1000, 1143.9)])
def test_the_draws_are_uniform_over_the_qualifying_cells(seed, M, limit):
    geom, starts, free = _strip(M)
    q = np.flatnonzero(free)
    # one set, k = 0, the counter running 0 .. 63999: a call a draw
    host = _Host(geom, starts, CELL, free, Layer(free), 1, 1, seed=seed)
    cells, uniforms = np.empty(DRAWS, np.int64), np.empty(DRAWS, F)
    for t in range(DRAWS):
        host()
        cells[t], uniforms[t] = host.out['cells'][0, 0, 0], host.out['uniforms'][0, 0, 0]
    assert int(host.counter[0, 0]) == DRAWS
    running = np.searchsorted(q, cells)
    assert np.array_equal(q[running], cells) and np.array_equal(running, draw_rule.rank(draw_rule.hash(seed, 0, np.arange(DRAWS), 0, 0), M))
    # 250 sets x 256 draws at one counter: one call
    got = _Host(geom, starts, CELL, free, Layer(free), 250, 256, seed=seed)()
    sets = np.searchsorted(q, got['cells'].reshape(-1))
    assert np.array_equal(q[sets], got['cells'].reshape(-1))
    for ranks, us in ((running, uniforms), (sets, got['uniforms'].reshape(-1))):
        value = _chi2(np.bincount(ranks, minlength=M), DRAWS)
        print(f'seed {seed} M {M}: chi-square {value:.1f} (limit {limit})')
        assert value < limit
    if M == 64:
        pairs = np.bincount((running[:-1]//8)*8 + running[1:]//8, minlength=64)
        value = _chi2(pairs, DRAWS - 1)
        print(f'seed {seed}: consecutive counters {value:.1f}')
        assert value < 103.4
        for ranks, us in ((running, uniforms), (sets, got['uniforms'].reshape(-1))):
            table = np.bincount((ranks//8)*8 + np.minimum((us*F(8)).astype(np.int64), 7), minlength=64)
            value = _chi2(table, DRAWS)
            print(f'seed {seed}: rank against uniform {value:.1f}')
            assert value < 103.4


# ---------------------------------------------------------------------------------------------------------------------
# header, loader, refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_the_header_declares_the_calls_and_the_loader_binds_them():
    from megastep_amd import _lib
    assert 'ms_nav_draws' in declared_symbols(('megastep_hip.h',)) and 'ms_host_nav_draws' in declared_symbols(('megastep_hip_test.h',))
    assert {'ms_nav_draws', 'ms_host_nav_draws'} <= set(_lib.SYMBOLS)
    text = open(os.path.join(ROOT, 'include', 'megastep_hip.h')).read()
    assert int(re.search(r'#define MS_ABI_VERSION (\d+)', text).group(1)) == _lib.ABI_VERSION
    handle = _lib.lib()
    assert hasattr(handle, 'ms_nav_draws') and hasattr(handle, 'ms_host_nav_draws')


def test_the_mirror_has_the_c_layout():
    import subprocess
    import tempfile
    from megastep_amd import _lib
    name = 'MsNavDraws'
    fields = ('source', 'gate', 'where', 'lo', 'hi', 'n_sets', 'n_draws', 'seed', 'counter', 'mask', 'cells', 'points', 'uniforms', 'values',
              'counts', 'max_cells')
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "megastep_hip.h"\nint main(){printf("%zu", sizeof(' + name + '));' +
           ''.join(f'printf(" %zu", offsetof({name}, {f}));' for f in fields) + '}')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, 't.c'), 'w').write(src)
        subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), os.path.join(d, 't.c'), '-o', os.path.join(d, 't')])
        got = list(map(int, subprocess.check_output([os.path.join(d, 't')]).split()))
    assert [f for f, _ in _lib.MsNavDraws._fields_] == list(fields)
    assert got == [ctypes.sizeof(_lib.MsNavDraws)] + [getattr(_lib.MsNavDraws, f).offset for f in fields]


def test_bad_arguments_are_refused_before_any_launch():
    from megastep_amd import _lib
    h = _lib.lib()
    fake = 64                                       # (never dereferenced: every call below fails its checks first)
    G, L, D = _lib.MsNavGrid, _lib.MsNavLayer, _lib.MsNavDraws
    grid = G(n_envs=2, cell=.125, clearance=.106, geom=fake, starts=fake, max_framed=100, free_cells=fake)
    ref = ctypes.byref

    def call(entry, draws=None, source=None, gate=None):
        src = dict(values=fake, is_float=0, n_fields=1, field=None)
        spec = dict(source=L(**{**src, **(source or {})}), gate=L(**gate) if gate else L(), where=1, lo=0., hi=1., n_sets=2, n_draws=7, seed=0,
                    counter=fake, mask=None, cells=fake, points=fake, uniforms=fake, values=None, counts=fake, max_cells=100)
        d = D(**{**spec, **(draws or {})})
        return entry(ref(grid), ref(d), None) if entry is h.ms_nav_draws else entry(ref(grid), ref(d))

    floats = dict(is_float=1)
    for entry in (h.ms_nav_draws, h.ms_host_nav_draws):
        for bad in (dict(n_draws=0), dict(n_draws=257), dict(n_draws=-1), dict(n_sets=0), dict(where=2), dict(counter=None), dict(cells=None),
                    dict(points=None), dict(uniforms=None), dict(counts=None), dict(counter=66), dict(cells=66), dict(points=66), dict(uniforms=66),
                    dict(counts=66), dict(values=fake), dict(max_cells=-1)):
            assert call(entry, draws=bad) == -1, bad
        for bad in (dict(lo=float('nan')), dict(hi=float('nan')), dict(values=66)):
            assert call(entry, draws=bad, source=floats) == -1, bad
        for bad in (dict(values=None), dict(is_float=2), dict(n_fields=0), dict(n_fields=3), dict(field=66), dict(is_float=1, values=66)):
            assert call(entry, source=bad) == -1, bad
        for bad in (dict(values=fake, is_float=1, n_fields=1), dict(values=fake, is_float=0, n_fields=3), dict(values=fake, is_float=0, n_fields=0)):
            assert call(entry, gate=bad) == -1, bad
        assert call(entry, draws=dict(max_cells=2**20 + 1)) == -3                    # (MS_EUNSUPPORTED: nothing enqueued)
    assert h.ms_nav_draws(None, None, None) == -1 and h.ms_host_nav_draws(ref(grid), None) == -1 and h.ms_nav_draws(ref(grid), None, None) == -1


def test_the_python_call_refuses_what_it_cannot_do():
    from megastep_amd import cuda
    geom = np.array([[0, 0, 8, 8], [0, 0, 8, 8]], np.int32)
    starts = np.array([0, 64, 128], np.int64)
    grid = cuda.NavGrid(torch.as_tensor(geom), torch.as_tensor(starts), torch.ones(128, dtype=torch.uint8), CELL, RADIUS, geom, starts)
    maps = cuda.seen_maps(grid, 3)
    floats = torch.zeros(128)
    with pytest.raises(RuntimeError, match='GPU'):
        cuda.cell_draws(grid, grid, 3, 7)
    for bad in (0, 257, -1, 2.):
        with pytest.raises(RuntimeError, match='n_draws'):
            cuda.cell_draws(grid, grid, 3, bad)
    for bad in (0, 1.5):
        with pytest.raises(RuntimeError, match='n_sets'):
            cuda.cell_draws(grid, grid, bad, 7)
    for bad in (-1, 2**64, 1.):
        with pytest.raises(RuntimeError, match='seed'):
            cuda.cell_draws(grid, grid, 3, 7, seed=bad)
    with pytest.raises(RuntimeError, match='gate'):
        cuda.cell_draws(grid, grid, 3, 7, gate=floats)
    for bounds in (dict(), dict(lo=1.), dict(hi=1.), dict(lo=float('nan'), hi=1.), dict(lo=0., hi=float('nan'))):
        with pytest.raises(RuntimeError, match='bounds'):
            cuda.cell_draws(grid, floats, 3, 7, **bounds)
    for bounds in (dict(lo=1.), dict(hi=1.), dict(lo=0., hi=1.)):
        with pytest.raises(RuntimeError, match='bounds'):
            cuda.cell_draws(grid, maps, 3, 7, **bounds)
    with pytest.raises(RuntimeError, match='entries'):
        cuda.cell_draws(grid, torch.zeros(100, dtype=torch.uint8), 3, 7)
    with pytest.raises(RuntimeError, match='entries'):
        cuda.cell_draws(grid, torch.zeros(100), 3, 7, lo=0., hi=1.)
    with pytest.raises(RuntimeError, match='one per view'):
        cuda.cell_draws(grid, maps, 2, 7)
    with pytest.raises(RuntimeError, match='one per view'):
        cuda.cell_draws(grid, grid, 2, 7, gate=maps)
    with pytest.raises(RuntimeError, match=r'\(N, P\)'):
        cuda.cell_draws(grid, cuda.cell_layer(maps, field=torch.zeros((2, 2), dtype=torch.int64)), 3, 7)
    with pytest.raises(RuntimeError, match=r'\(N, P\)'):
        cuda.cell_draws(grid, grid, 3, 7, gate=cuda.cell_layer(maps, field=torch.zeros((3, 3), dtype=torch.int64)))
    for bad in (torch.zeros((2, 3), dtype=torch.uint8), torch.zeros((2, 2), dtype=torch.bool), 'x'):
        with pytest.raises(RuntimeError, match='mask'):
            cuda.cell_draws(grid, grid, 3, 7, mask=bad)
    # a mis-shaped out: another K, another P, the values of the other kind of source, another grid, not a CellDraws
    new = lambda p, k, values, grid=grid: cuda.CellDraws(grid, p, k, torch.zeros((2, p, k), dtype=torch.int32), torch.zeros(2, p, k, 2),
                                                         torch.zeros(2, p, k), torch.zeros(2, p, k) if values else None,
                                                         torch.zeros((2, p), dtype=torch.int32), torch.zeros((2, p), dtype=torch.int32))
    other = cuda.NavGrid(torch.as_tensor(geom), torch.as_tensor(starts), torch.ones(128, dtype=torch.uint8), CELL, RADIUS, geom, starts)
    for bad in (new(3, 8, False), new(2, 7, False), new(3, 7, True), new(3, 7, False, other), 'x', torch.zeros(2, 3, 7)):
        with pytest.raises(RuntimeError, match='out'):
            cuda.cell_draws(grid, grid, 3, 7, out=bad)
    with pytest.raises(RuntimeError, match='out'):
        cuda.cell_draws(grid, floats, 3, 7, lo=0., hi=1., out=new(3, 7, False))
    with pytest.raises(RuntimeError, match='GPU'):
        cuda.cell_draws(grid, grid, 3, 7, out=new(3, 7, False))                 # (a fitting out gets as far as the launch)
