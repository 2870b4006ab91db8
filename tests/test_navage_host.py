"""Age maps (`ms_nav_ages`, `cuda.age_maps`, `AgeMaps.mark`, `modules.Idleness`, `demo.Patrol`) on the CPU: the contract of
include/megastep_hip.h (MsNavAges) restated in numpy (`age_rule`, built on `seen_rule.marks` for which cells a call marks, and
which tests/test_gpu_navage.py holds the kernel to, exactly); the host instantiation of the kernel's own functions against the
rule over sequences of calls; a known answer written out by hand; the clock at its cap; consistency with the seen maps and the
seeded fields; and the C-ABI's declarations, layout and refusals."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import test_abi
from tests.test_abi import ROOT, declared_symbols
from tests.test_navfield_host import CELL, RADIUS, F
from tests.test_navseed_host import host_field
from tests.test_navseen_host import _host as seen_host, cases, seen_rule

INF, NAN = F(np.inf), F(np.nan)
CAP = 2**24


class age_rule:
    """The contract in numpy, one operation per statement, in the order the header gives. A map's state is `last` (S, ny, nx)
    float32 and `clock` (S,) int32."""

    @staticmethod
    def survey(countable, last, now, threshold):
        """The survey of one env's maps: last (S, cells) and now (S,) -> dict of oldest, total_age, n_stale, stale, ages."""
        S = len(last)
        counts = (np.asarray(countable).reshape(-1).astype(np.uint8) & 1).astype(bool)
        ticks = last.astype(np.int64)
        age = np.asarray(now, np.int64)[:, None] - ticks
        old = age >= threshold
        stale = old & counts[None]
        counted = age[:, counts]
        oldest = np.maximum(counted.max(1, initial=0), 0)
        return dict(oldest=oldest.astype(np.int32), total_age=counted.sum(1).astype(np.int64), n_stale=stale.sum(1).astype(np.int32),
                    stale=stale.astype(np.uint8).reshape(S, -1), ages=age.astype(F).reshape(S, -1))

    @staticmethod
    def call(geom, cell, countable, last, clock, origins=None, dirs=None, distances=None, slot=None, max_range=10., reset=None,
             advance=True, threshold=64, survey=True):
        """One call for one env: (last, clock) as they were -> dict(last, clock, swept, gained, idle[, the survey's])."""
        jx0, iy0, nx, ny = geom
        S = len(last)
        shape = np.shape(last)
        last, clock = np.array(last, F).reshape(S, -1), np.array(clock, np.int32)
        clear = np.zeros(S, bool) if reset is None else np.asarray(reset).astype(bool)
        last[clear] = 0
        clock[clear] = 0
        ticked = np.minimum(clock.astype(np.int64) + 1, CAP)
        now = ticked if advance else clock.astype(np.int64)
        swept, gained, idle = np.zeros(S, np.int32), np.zeros(S, np.int32), np.zeros(S, np.int64)
        counts = (np.asarray(countable).reshape(-1).astype(np.uint8) & 1).astype(bool)
        cells = nx*ny if nx > 0 and ny > 0 else 0
        if advance and cells > 0:
            viewer, _, _, at = seen_rule.marks(geom, cell, origins, dirs, distances, max_range)
            slot = np.arange(len(origins)) if slot is None else np.asarray(slot)
            for s in range(S):
                marked = np.unique(at[slot[viewer] == s])                # a set: a cell is in it once
                before = last[s, marked]
                ticks = before.astype(np.int64)
                age = now[s] - ticks
                last[s, marked] = F(now[s])
                counted = counts[marked]
                swept[s] = counted.sum()
                gained[s] = (counted & (before == 0)).sum()
                idle[s] = age[counted].sum()
        out = dict(last=last.reshape(shape), clock=now.astype(np.int32), swept=swept, gained=gained, idle=idle)
        if survey:
            found = age_rule.survey(counts if cells > 0 else np.zeros(0, bool), last[:, :cells], now, threshold)
            found['stale'], found['ages'] = found['stale'].reshape(shape), found['ages'].reshape(shape)
            out.update(found)
        return out


_SPARE = np.zeros(8, np.float64)         # (somewhere to point for an env without cells)
COUNTS = ('swept', 'gained', 'idle')
SURVEY = ('oldest', 'total_age', 'n_stale', 'stale', 'ages')


def host(geom, cell, countable, last, clock, origins=None, dirs=None, distances=None, slot=None, max_range=10., reset=None, advance=True,
         threshold=64, survey=True, status=0):
    """ms_host_nav_ages on copies: the dict age_rule.call returns."""
    from megastep_amd import _lib
    S = len(last)
    geom = np.array(geom, np.int32)
    countable = np.ascontiguousarray(countable, np.uint8)
    last, clock = np.array(last, F), np.array(clock, np.int32)
    out = dict(last=last, clock=clock, swept=np.full(S, -7, np.int32), gained=np.full(S, -7, np.int32), idle=np.full(S, -7, np.int64))
    if survey:
        out.update(oldest=np.full(S, -7, np.int32), total_age=np.full(S, -7, np.int64), n_stale=np.full(S, -7, np.int32),
                   stale=np.full(last.shape, 9, np.uint8), ages=np.full(last.shape, -7., F))
    given = [None if a is None else np.ascontiguousarray(a, F) for a in (origins, dirs, distances)]
    slot = None if slot is None else np.ascontiguousarray(slot, np.int32)
    reset = None if reset is None else np.ascontiguousarray(reset, np.uint8)
    ptr = lambda a: None if a is None else (a.ctypes.data or _SPARE.ctypes.data)
    P, R = given[2].shape if given[2] is not None else (0, 0)
    spec = _lib.MsNavAges(S, P, R, ptr(given[0]), ptr(given[1]), ptr(given[2]), ptr(slot), max_range, ptr(reset), ptr(countable), int(advance),
                          threshold, ptr(last), ptr(clock), *(ptr(out[k]) for k in COUNTS), *(ptr(out.get(k)) for k in SURVEY), 0)
    assert _lib.lib().ms_host_nav_ages(ptr(geom), cell, ctypes.byref(spec)) == status
    return out


def same(geom, countable, last, clock, *rays, cell=CELL, **kw):
    want = age_rule.call(geom, cell, countable, last, clock, *rays, **kw)
    got = host(geom, cell, countable, last, clock, *rays, **kw)
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert np.array_equal(got[k], want[k]), (k, got[k], want[k])
    return want


def fans(rng, centres, R, reach):
    """(origins (P, 2), dirs (P, R, 2), distances (P, R)) made up: fans of R rays of any length round `centres` (P, 2)."""
    p = len(centres)
    angle = rng.uniform(0, 2*np.pi, (p, 1)) + np.linspace(0, 2., R)[None]
    dirs = (np.stack([np.cos(angle), np.sin(angle)], -1)*rng.uniform(.5, 2., (p, R, 1))).astype(F)
    return np.asarray(centres, F), dirs, rng.uniform(.1, reach, (p, R)).astype(F)


def sequence(case, rng, S):
    """Seven calls' (rays, keywords) for a case: six with rays - rendered ones and fans, a reset in the middle, short rays, skipped
    viewers - and a survey alone."""
    slot = None if S == 2 else [0, 0]
    rendered = (case.origins, case.dirs, case.distances)
    yield rendered, dict(slot=slot)
    yield fans(rng, case.origins + rng.uniform(-.3, .3, (2, 2)), 48, 6.), dict(slot=slot, survey=False)
    yield fans(rng, case.origins + rng.uniform(-.3, .3, (2, 2)), 48, 6.), dict(slot=slot, max_range=2.)
    yield rendered, dict(slot=slot, reset=[1, 0][:S], max_range=3.)
    yield fans(rng, case.origins, 17, 3.), dict(slot=[1, 0] if S == 2 else [0, -1], threshold=2)
    yield (), dict(advance=False, threshold=2)
    yield rendered, dict(slot=slot, threshold=3)


@pytest.mark.parametrize('S', [2, 1])
def test_the_host_instantiation_is_the_rule_over_a_sequence_of_calls(S):
    swept = 0
    for case in cases():
        rng = np.random.RandomState(41)
        last, clock = np.zeros((S,) + case.free.shape, F), np.zeros(S, np.int32)
        before = None
        for k, (rays, kw) in enumerate(sequence(case, rng, S)):
            got = same(case.geom, case.free, last, clock, *rays, **kw)
            if k == 0:
                assert (got['gained'] > 0).all() and got['gained'].sum() > 100 and got['gained'].tolist() == got['swept'].tolist() == got['idle'].tolist()
                assert got['oldest'].tolist() == [1]*S and (got['n_stale'] == 0).all()
                assert got['total_age'].tolist() == (case.free.sum() - got['swept']).tolist()
            if k == 3:
                assert got['clock'].tolist() == [1, 4][:S] and got['gained'][0] == got['swept'][0] and (got['last'][0] <= 1).all()
            if k == 5:                                                   # the survey alone: nothing moved, and the ages are those of call 4
                assert np.array_equal(got['last'], last) and np.array_equal(got['clock'], clock) and not got['swept'].any()
                assert all(np.array_equal(got[name], before[name]) for name in SURVEY)
            assert (got['gained'] <= got['swept']).all() and (got['idle'] >= got['gained']).all()
            swept += int(got['swept'].sum())
            last, clock, before = got['last'], got['clock'], got
        assert clock.tolist() == [3, 6][:S] and (before['n_stale'] > 0).all() and (before['oldest'] == clock).all()
        # the numbers hang together: the ages are the clock less the ticks, the stale cells those the byte store names
        assert np.array_equal(before['ages'], clock[:, None, None] - last)
        assert before['n_stale'].tolist() == [int(m.sum()) for m in before['stale']]
        assert not (before['stale'].astype(bool) & ~case.free).any()
    assert swept > 10000


def test_a_known_answer_by_hand():
    """A 5 x 1 grid of unit cells from x = 0; the ray from (0.5, 0.5) along +x for 2 m passes over cells 0, 1 and 2, and one from
    (3.5, 0.5) for 1 m over cells 3 and 4. Cell 1 does not count."""
    geom, countable = (0, 0, 5, 1), np.array([[1, 0, 1, 1, 1]], np.uint8)
    left = (np.array([[.5, .5]], F), np.array([[[1., 0.]]], F), np.array([[2.]], F))
    right = (np.array([[3.5, .5]], F), np.array([[[2., 0.]]], F), np.array([[1.]], F))
    blank = np.zeros((1, 1, 5), F)
    a = same(geom, countable, blank, [0], *left, cell=1., threshold=2)
    assert a['last'].tolist() == [[[1., 1., 1., 0., 0.]]] and a['clock'].tolist() == [1]
    assert (a['swept'].tolist(), a['gained'].tolist(), a['idle'].tolist()) == ([2], [2], [2])
    assert (a['oldest'].tolist(), a['total_age'].tolist(), a['n_stale'].tolist()) == ([1], [2], [0])
    assert a['ages'].tolist() == [[[0., 0., 0., 1., 1.]]] and a['stale'].tolist() == [[[0, 0, 0, 0, 0]]]
    b = same(geom, countable, a['last'], a['clock'], *right, cell=1., threshold=2)
    assert b['last'].tolist() == [[[1., 1., 1., 2., 2.]]] and b['clock'].tolist() == [2]
    assert (b['swept'].tolist(), b['gained'].tolist(), b['idle'].tolist()) == ([2], [2], [4])
    assert (b['oldest'].tolist(), b['total_age'].tolist(), b['n_stale'].tolist()) == ([1], [2], [0])
    c = same(geom, countable, b['last'], b['clock'], *right, cell=1., threshold=2)
    assert c['last'].tolist() == [[[1., 1., 1., 3., 3.]]] and c['clock'].tolist() == [3]
    assert (c['swept'].tolist(), c['gained'].tolist(), c['idle'].tolist()) == ([2], [0], [2])
    assert (c['oldest'].tolist(), c['total_age'].tolist(), c['n_stale'].tolist()) == ([2], [4], [2])
    assert c['ages'].tolist() == [[[2., 2., 2., 0., 0.]]] and c['stale'].tolist() == [[[1, 0, 1, 0, 0]]]


def test_two_viewers_over_the_same_cell_count_it_once():
    geom, countable = (0, 0, 5, 1), np.ones((1, 5), np.uint8)
    origins, dirs, distances = np.array([[.5, .5], [2.5, .5]], F), np.array([[[1., 0.]], [[-1., 0.]]], F), np.array([[2.], [2.]], F)
    got = same(geom, countable, np.zeros((1, 1, 5), F), [6], origins, dirs, distances, slot=[0, 0], cell=1.)
    assert got['last'].tolist() == [[[7., 7., 7., 0., 0.]]]
    assert (got['swept'].tolist(), got['gained'].tolist(), got['idle'].tolist()) == ([3], [3], [21])
    # ... as do the many samples of one ray that fall in a cell, and a ray run twice
    twice = same(geom, countable, np.zeros((1, 1, 5), F), [6], origins[[0, 0]], dirs[[0, 0]], distances[[0, 0]], slot=[0, 0], cell=1.)
    assert np.array_equal(twice['last'], got['last']) and twice['idle'].tolist() == [21]


def test_the_clock_stops_at_two_to_the_24_and_ages_stay_exact():
    case = cases()[1]
    rays = (case.origins, case.dirs, case.distances)
    last = np.zeros((2,) + case.free.shape, F)
    last[1][::2] = F(CAP - 3)
    clock = np.array([CAP - 2, CAP - 2], np.int32)
    ticks = []
    for k in range(3):
        got = same(case.geom, case.free, last, clock, *rays, threshold=CAP)
        ticks.append(got['clock'].tolist())
        marked = got['last'] == F(got['clock'][0])
        assert marked[0].sum() > 100 and (got['ages'][marked] == 0).all()
        assert set(np.unique(got['ages'][0][~marked[0]]).tolist()) == {float(got['clock'][0])}      # (never seen: its whole clock)
        assert got['oldest'].tolist() == [got['clock'][0]]*2 and (got['n_stale'] > 0).all() == (k > 0)
        last, clock = got['last'], got['clock']
    assert ticks == [[CAP - 1]*2, [CAP]*2, [CAP]*2]
    assert got['idle'].tolist() == [0, 0] and (got['swept'] > 100).all()      # (at the cap a cell re-seen has age 0)
    assert got['total_age'][0] == CAP*int((case.free & ~marked[0]).sum())


def test_without_advance_the_maps_stand_and_reset_still_clears():
    case = cases()[2]
    rays = (case.origins, case.dirs, case.distances)
    first = same(case.geom, case.free, np.zeros((2,) + case.free.shape, F), [4, 9], *rays, threshold=5)
    still = same(case.geom, case.free, first['last'], first['clock'], advance=False, threshold=5)
    assert np.array_equal(still['last'], first['last']) and still['clock'].tolist() == [5, 10]
    assert all(np.array_equal(still[k], first[k]) for k in SURVEY) and not still['idle'].any()
    assert first['n_stale'][0] > 0 and first['oldest'].tolist() == [5, 10]
    cleared = same(case.geom, case.free, first['last'], first['clock'], advance=False, reset=[0, 1], threshold=5)
    assert not cleared['last'][1].any() and cleared['clock'].tolist() == [5, 0] and cleared['oldest'].tolist() == [5, 0]
    assert np.array_equal(cleared['last'][0], first['last'][0])
    # without the survey's outputs only the marks run
    bare = same(case.geom, case.free, first['last'], first['clock'], *rays, survey=False)
    assert sorted(bare) == ['clock', 'gained', 'idle', 'last', 'swept'] and bare['gained'].tolist() == [0, 0]
    assert bare['idle'].tolist() == bare['swept'].tolist()


def test_odd_rays_and_an_env_without_cells():
    case = cases()[3]
    origins, dirs, distances = case.origins.copy(), case.dirs.copy(), case.distances.copy()
    distances[0, :8] = [INF, 0., -1., NAN, -INF, F(1e-30), F(3e38), F(2.5)]
    dirs[0, 8:14] = [[NAN, 1.], [1., INF], [0., 0.], [-INF, NAN], [3e38, 3e38], [1e-30, 1e-30]]
    origins[1] = [NAN, 1.]
    blank = np.zeros((2,) + case.free.shape, F)
    got = same(case.geom, case.free, blank, [0, 0], origins, dirs, distances)
    assert got['swept'][0] > 20 and got['swept'][1] == 0 and got['clock'].tolist() == [1, 1]
    none = np.zeros((2, 0, 0), F)
    for geom in ((0, 0, 0, 0), (3, 4, 0, 7)):
        got = same(geom, np.zeros(0, np.uint8), none, [5, 6], case.origins, case.dirs, case.distances, reset=[0, 1])
        assert got['clock'].tolist() == [6, 1] and not got['swept'].any() and not got['oldest'].any() and not got['total_age'].any()
        assert same(geom, np.zeros(0, np.uint8), none, [5, 6], advance=False)['clock'].tolist() == [5, 6]


@pytest.mark.parametrize('nx,ny', [(1, 1), (1, 40), (40, 1), (31, 1), (32, 1), (33, 1), (7, 9), (8, 8), (13, 5)])
def test_small_grids_at_the_bitmasks_word_edges(nx, ny):
    rng = np.random.RandomState(nx*100 + ny)
    geom = (-2, 3, nx, ny)
    countable = (rng.rand(ny, nx) < .8).astype(np.uint8)
    last, clock = np.zeros((2, ny, nx), F), np.zeros(2, np.int32)
    centres = (np.array([[-2, 3], [-3 + nx, 2 + ny]]) + .5 + rng.uniform(-.3, .3, (2, 2)))*CELL       # (inside the first and the last cell)
    for k in range(4):
        got = same(geom, countable, last, clock, *fans(rng, centres, 9, 1. + CELL*(nx + ny)), threshold=2, reset=[k == 2, 0])
        last, clock = got['last'], got['clock']
    assert clock.tolist() == [2, 4] and last.max() == 4.


def test_the_ticks_are_the_seen_maps_bits_and_gained_is_their_gained():
    for case in cases()[::2]:
        rng = np.random.RandomState(43)
        last, clock = np.zeros((2,) + case.free.shape, F), np.zeros(2, np.int32)
        maps, totals = case.blank, np.zeros(2, np.int32)
        calls = 0
        for rays, kw in sequence(case, rng, 2):
            if not rays:
                continue
            got = host(case.geom, CELL, case.free, last, clock, *rays, **kw)
            seen = {k: v for k, v in kw.items() if k in ('slot', 'max_range', 'reset')}
            maps, gained, totals = seen_host(case.geom, CELL, case.free, maps, totals, *rays, **seen)
            assert np.array_equal(got['last'] > 0, maps.astype(bool)) and got['gained'].tolist() == gained.tolist()
            last, clock = got['last'], got['clock']
            calls += 1
        assert calls == 6 and totals.sum() > 200


def test_the_stale_bytes_seed_the_field_of_the_rules_marks():
    for case in cases()[1::2]:
        rays = (case.origins, case.dirs, case.distances)
        state = host(case.geom, CELL, case.free, np.zeros((2,) + case.free.shape, F), [0, 0], *rays, threshold=1, max_range=3.)
        state = host(case.geom, CELL, case.free, state['last'], state['clock'], *fans(np.random.RandomState(3), case.origins, 30, 4.), threshold=1)
        want = age_rule.call(case.geom, CELL, case.free, state['last'], state['clock'], advance=False, threshold=1)
        for s in range(2):
            marks = ((want['clock'][s] - want['last'][s].astype(np.int64) >= 1) & case.free).astype(np.uint8)
            assert 0 < marks.sum() < case.free.sum()
            got, n_got, _ = host_field(case.geom, CELL, case.free, state['stale'][s], True)
            expected, n_expected, _ = host_field(case.geom, CELL, case.free, marks, True)
            assert n_got == n_expected == marks.sum() and got.tobytes() == expected.tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# header, loader, refusals
# ---------------------------------------------------------------------------------------------------------------------
FIELDS = ('n_maps', 'n_viewers', 'n_rays', 'origins', 'dirs', 'distances', 'slot', 'max_range', 'reset', 'countable', 'advance', 'threshold',
          'last', 'clock', 'swept', 'gained', 'idle', 'oldest', 'total_age', 'n_stale', 'stale', 'ages', 'max_cells')


def test_the_header_declares_the_call_and_the_loader_binds_it():
    from megastep_amd import _lib
    assert 'ms_nav_ages' in declared_symbols(('megastep_hip.h',)) and 'ms_host_nav_ages' in declared_symbols(('megastep_hip_test.h',))
    assert {'ms_nav_ages', 'ms_host_nav_ages'} <= set(_lib.SYMBOLS)
    text = open(os.path.join(ROOT, 'include', 'megastep_hip.h')).read()
    assert int(re.search(r'#define MS_ABI_VERSION (\d+)', text).group(1)) == _lib.ABI_VERSION == 17
    handle = _lib.lib()
    assert hasattr(handle, 'ms_nav_ages') and hasattr(handle, 'ms_host_nav_ages') and handle.ms_abi_version() == 17


def test_the_mirror_has_the_c_layout():
    from megastep_amd import _lib
    text = open(os.path.join(ROOT, 'include', 'megastep_hip.h')).read()
    assert 'MsNavAges' in re.findall(r'^\}\s*(Ms\w+)\s*;', text, flags=re.M)
    assert [f for f, _ in _lib.MsNavAges._fields_] == list(FIELDS)
    test_abi.test_struct_layouts_match_the_header()             # (every mirror's size and offsets against a C compile of the header)


def test_bad_arguments_are_refused_before_any_launch():
    from megastep_amd import _lib
    h = _lib.lib()
    fake = 64                                       # (never dereferenced: every call below fails its checks first)
    grid = dict(n_envs=2, cell=.125, clearance=.106, geom=fake, starts=fake, max_framed=100, free_cells=fake)
    ages = dict(n_maps=2, n_viewers=2, n_rays=8, origins=fake, dirs=fake, distances=fake, slot=None, max_range=10., reset=None,
                countable=None, advance=1, threshold=64, last=fake, clock=fake, swept=fake, gained=fake, idle=fake, oldest=fake,
                total_age=fake, n_stale=fake, stale=fake, ages=fake, max_cells=64)
    G, V = _lib.MsNavGrid, _lib.MsNavAges
    ref = ctypes.byref
    assert h.ms_nav_ages(None, ref(V(**ages)), None) == -1 and h.ms_nav_ages(ref(G(**grid)), None, None) == -1
    for bad in (dict(n_envs=0), dict(cell=0.), dict(geom=None), dict(starts=None), dict(free_cells=None), dict(geom=68)):
        assert h.ms_nav_ages(ref(G(**{**grid, **bad})), ref(V(**ages)), None) == -1, bad
    for bad in (dict(last=None), dict(clock=None), dict(threshold=0), dict(threshold=-3), dict(n_viewers=0), dict(n_maps=0), dict(n_rays=0),
                dict(n_viewers=3), dict(n_maps=3), dict(origins=None), dict(dirs=None), dict(distances=None), dict(origins=68), dict(dirs=68),
                dict(distances=66), dict(slot=66), dict(last=66), dict(clock=66), dict(swept=66), dict(gained=66), dict(idle=68), dict(oldest=66),
                dict(total_age=68), dict(n_stale=66), dict(ages=66), dict(advance=2), dict(advance=-1), dict(max_range=0.),
                dict(max_range=float('inf')), dict(max_range=float('nan')), dict(max_cells=-1)):
        assert h.ms_nav_ages(ref(G(**grid)), ref(V(**{**ages, **bad})), None) == -1, bad
    # an env of more than 2^20 cells: unsupported, and nothing is enqueued
    assert h.ms_nav_ages(ref(G(**grid)), ref(V(**{**ages, 'max_cells': 2**20 + 1})), None) == -3
    # the host instantiation refuses the same, and a grid of its own that is too large
    case = cases()[0]
    blank = np.zeros((2,) + case.free.shape, F)
    for bad in (dict(threshold=0), dict(max_range=0.), dict(slot=None, origins=case.origins[:1], dirs=case.dirs[:1], distances=case.distances[:1])):
        host(case.geom, CELL, case.free, blank, [0, 0], **{**dict(origins=case.origins, dirs=case.dirs, distances=case.distances), **bad}, status=-1)
    host(case.geom, CELL, case.free, blank, [0, 0], advance=True, status=-1)                       # (no viewers, and the clock to tick)
    host((0, 0, 1025, 1024), CELL, case.free, blank, [0, 0], advance=False, status=-3)
    spec = _lib.MsNavAges(n_maps=1, max_range=10., threshold=1, last=fake, clock=fake)
    assert h.ms_host_nav_ages(None, CELL, ref(spec)) == -1 and h.ms_host_nav_ages(np.zeros(4, np.int32).ctypes.data, CELL, None) == -1
    assert h.ms_host_nav_ages(np.zeros(4, np.int32).ctypes.data, CELL, ref(spec)) == -1            # (no countable)


def _grid(cuda):
    geom = np.array([[0, 0, 8, 8], [0, 0, 8, 8]], np.int32)
    starts = np.array([0, 64, 128], np.int64)
    return cuda.NavGrid(torch.as_tensor(geom), torch.as_tensor(starts), torch.ones(128, dtype=torch.uint8), CELL, RADIUS, geom, starts)


def test_the_python_calls_refuse_what_they_cannot_do():
    from megastep_amd import cuda
    grid = _grid(cuda)
    ages = cuda.age_maps(grid, 2)
    assert ages.last.shape == (256,) and ages.last.dtype == torch.float32 and ages.clock.shape == (2, 2) and ages.clock.dtype == torch.int32
    assert ages.n_countable.tolist() == [64, 64] and ages.threshold == 64 and ages.stale.dtype == torch.uint8 and ages.ages.shape == (256,)
    assert ages.total_age.dtype == torch.int64 and ages.oldest.shape == ages.n_stale.shape == (2, 2)
    assert ages.image(1, 1).shape == ages.age_image(1, 1).shape == ages.stale_image(1, 1).shape == (8, 8)
    assert ages.stale_image(1, 1).dtype == torch.bool and ages.mean_age().tolist() == [[0., 0.], [0., 0.]]
    half = torch.ones(128, dtype=torch.bool)
    half[:32] = False
    assert cuda.age_maps(grid, 1, countable=half, threshold=1).n_countable.tolist() == [32, 64]
    assert cuda.age_maps(grid, 1, ages=False).ages is None
    for bad in (0, 2.5):
        with pytest.raises(RuntimeError, match='n_maps'):
            cuda.age_maps(grid, bad)
    for bad in (0, -1, 2.5, True):
        with pytest.raises(RuntimeError, match='threshold'):
            cuda.age_maps(grid, 1, threshold=bad)
    with pytest.raises(RuntimeError, match='countable'):
        cuda.age_maps(grid, 1, countable=torch.ones(64, dtype=torch.uint8))
    o, d, t = torch.zeros(2, 2, 2), torch.ones(2, 2, 8, 2), torch.ones(2, 2, 8)
    with pytest.raises(RuntimeError, match='GPU'):
        ages.mark(o, d, t)
    with pytest.raises(RuntimeError, match='GPU'):
        ages.survey()
    with pytest.raises(RuntimeError, match=r'\(N, P, R, 2\)'):
        ages.mark(torch.zeros(3, 2, 2), d, t)
    with pytest.raises(RuntimeError, match=r'\(N, P, R, 2\)'):
        ages.mark(o, d, torch.ones(2, 2, 7))
    with pytest.raises(RuntimeError, match='dtype'):
        ages.mark(o.double(), d, t)
    with pytest.raises(RuntimeError, match='one per map'):
        ages.mark(torch.zeros(2, 3, 2), torch.ones(2, 3, 8, 2), torch.ones(2, 3, 8))
    with pytest.raises(RuntimeError, match='integer'):
        ages.mark(o, d, t, slot=torch.zeros(2, 2))
    with pytest.raises(RuntimeError, match='bool'):
        ages.mark(o, d, t, reset=torch.zeros(2, 2))
    for bad in (0., -1., float('inf'), float('nan')):
        with pytest.raises(RuntimeError, match='max_range'):
            ages.mark(o, d, t, max_range=bad)
    big = np.array([[0, 0, 1025, 1024]], np.int32)
    huge = cuda.NavGrid(torch.as_tensor(big), torch.tensor([0, 1025*1024]), torch.ones(1, dtype=torch.uint8), CELL, RADIUS, big,
                        np.array([0, 1025*1024], np.int64))
    with pytest.raises(RuntimeError, match='cells'):
        cuda.age_maps(huge, 1)


def test_age_maps_are_a_float_layer_of_ages_and_a_byte_layer_of_stale_cells():
    from megastep_amd import cuda
    from megastep_amd.nav import _layer
    grid = _grid(cuda)
    ages = cuda.age_maps(grid, 2)
    layer = cuda.cell_layer(ages)
    assert layer.is_float and layer.n_fields == 2 and layer.values.data_ptr() == ages.ages.data_ptr()
    assert _layer(ages).values.data_ptr() == ages.ages.data_ptr()
    gate = _layer(ages, byte=True)
    assert not gate.is_float and gate.n_fields == 2 and gate.values.data_ptr() == ages.stale.data_ptr()
    channel = cuda.map_channel(ages, scale=1/64)
    assert channel.source.values.data_ptr() == ages.ages.data_ptr() and channel.scale == 1/64
    gated = cuda.map_channel(grid, gate=ages)
    assert gated.gate.values.data_ptr() == ages.stale.data_ptr()
    with pytest.raises(RuntimeError, match='scale'):
        cuda.map_channel(ages)
    ages.stale[:5] = 1
    costs = cuda.mark_costs(ages, on=7., off=2.)
    assert costs.shape == ages.stale.shape and costs[:5].tolist() == [7.]*5 and costs[5:].eq(2.).all()
    with pytest.raises(RuntimeError, match='ages=False'):
        cuda.cell_layer(cuda.age_maps(grid, 1, ages=False))
