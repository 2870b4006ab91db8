"""The host statements of the scent fields (ms_host_nav_scent, ms_host_nav_scent_query: the kernels' own per-cell functions swept
serially, csrc/kernels/navscent.h) against tests/scent_rule.py, AS BITS; no GPU."""
import ctypes as C
import types
import numpy as np
import pytest
from tests.scent_rule import F, scent_rule, sniff_rule

CELL = .125
bits = lambda a: np.ascontiguousarray(a, F).view(np.uint32)
_p = lambda a: None if a is None else a.ctypes.data


def hand():
    """(6, 7) bool: a closed cell next to the frame (0, 1), a one-cell-wide corridor (rows 2-3, column 3), an isolated open cell (5, 6)."""
    return np.array([[1, 0, 1, 1, 1, 1, 1], [1, 1, 1, 1, 1, 1, 1], [0, 0, 0, 1, 0, 0, 0], [0, 0, 0, 1, 0, 0, 0], [1, 1, 1, 1, 1, 0, 0],
                     [1, 1, 1, 1, 1, 0, 1]], bool)


def world(envs, G, cell=CELL):
    """Envs [(geom, free (ny, nx) bool)] with G empty stores each: the ragged arrays of the C-ABI and the rule's per-env stores."""
    geom = np.array([g for g, _ in envs], np.int32)
    starts = np.concatenate([[0], np.cumsum(geom[:, 2].astype(np.int64)*geom[:, 3])]).astype(np.int64)
    free = np.concatenate([f.reshape(-1).astype(np.uint8) for _, f in envs] + [np.zeros(1, np.uint8)])
    framed = [(g[2] + 2)*(g[3] + 2) for g in geom if g[2] > 0 and g[3] > 0]
    size = max(G*int(starts[-1]), 1)
    return types.SimpleNamespace(envs=envs, G=G, cell=cell, geom=geom, starts=starts, free=free, max_framed=max(framed, default=0), V=np.zeros(size, F),
                                 ws=np.zeros(size, F), peaks=np.full((len(envs), G), -1, F), scented=np.full((len(envs), G), -1, np.int32),
                                 rule=[np.zeros((G,) + f.shape, F) for _, f in envs])


def structs(w, points, amounts, field, reset, mask, rate, keep, floor, T):
    from megastep_amd import _lib
    grid = _lib.MsNavGrid(len(w.envs), w.cell, .1 if w.cell < .14 else w.cell, w.geom.ctypes.data, w.starts.ctypes.data, w.max_framed, w.free.ctypes.data)
    return grid, _lib.MsNavScent(w.G, 0 if points is None else points.shape[1], _p(points), _p(amounts), _p(field), _p(reset), _p(mask), rate, keep,
                                 floor, T, w.V.ctypes.data, w.ws.ctypes.data, w.peaks.ctypes.data, w.scented.ctypes.data)


def rule_tick(w, points=None, amounts=None, field=None, reset=None, mask=None, rate=.2, keep=.98, floor=1e-6, T=3):
    """One tick of the rule on w.rule; returns (the flat store, peaks, scented) as the C-ABI lays them out, masked-out summaries as `w` holds them."""
    peaks, scented = w.peaks.copy(), w.scented.copy()
    for e, (g, free) in enumerate(w.envs):
        none = np.zeros((0, 2), F)
        w.rule[e], pk, sc = scent_rule(g, w.cell, free, w.rule[e], none if points is None else points[e], None if points is None else amounts[e],
                                       None if field is None else field[e], rate, keep, floor, T, None if reset is None else reset[e],
                                       None if mask is None else mask[e])
        for k in range(w.G):
            if pk[k] is not None:
                peaks[e, k], scented[e, k] = pk[k], sc[k]
    return np.concatenate([v.reshape(-1) for v in w.rule] + [np.zeros(max(1 - w.G*int(w.starts[-1]), 0), F)]), peaks, scented


def tick(w, run, **call):
    """A tick by `run.tick` - into w.V, w.peaks and w.scented - and by the rule, equal as bits; no sign bit, no NaN, closed cells 0.f."""
    want, peaks, scented = rule_tick(w, **call)
    args = {k: call.get(k) for k in ('points', 'amounts', 'field', 'reset', 'mask')}
    args['reset'], args['mask'] = (None if a is None else np.ascontiguousarray(a, np.uint8) for a in (args['reset'], args['mask']))
    assert run.tick(w, *args.values(), call.get('rate', .2), call.get('keep', .98), call.get('floor', 1e-6), call.get('T', 3)) == 0
    assert np.array_equal(bits(w.V), bits(want)) and np.array_equal(bits(w.peaks), bits(peaks)) and np.array_equal(w.scented, scented)
    assert not (bits(w.V) >> 31).any() and not np.isnan(w.V).any() and not np.isnan(w.peaks).any()
    assert all(not v[:, ~free].any() for v, (_, free) in zip(w.rule, w.envs))
    return w


def sniff(w, run, points, field=None):
    """The query by `run.sniff` of the store the last tick left, equal to the rule's as bits."""
    n, p = points.shape[:2]
    out, grads = np.full((n, p), 7, F), np.full((n, p, 2), 7, F)
    assert run.sniff(w, points, field, out, grads) == 0
    for e, (g, free) in enumerate(w.envs):
        v, d = sniff_rule(g, w.cell, free, w.rule[e], points[e], None if field is None else field[e])
        assert np.array_equal(bits(out[e]), bits(v)) and np.array_equal(bits(grads[e]), bits(d)), e
    return out, grads


def host_call(grid, spec):
    from megastep_amd import _lib
    return getattr(_lib.lib(), 'ms_host_nav_scent' + ('_query' if isinstance(spec, _lib.MsNavScentQuery) else ''))(C.byref(grid), C.byref(spec))


def host_sniff(w, points, field, out, grads):
    from megastep_amd import _lib
    query = _lib.MsNavScentQuery(points.shape[1], points.ctypes.data, _p(field), w.V.ctypes.data, w.G, out.ctypes.data, grads.ctypes.data)
    return host_call(structs(w, None, None, None, None, None, .2, .9, 0., 1)[0], query)


host = types.SimpleNamespace(tick=lambda w, *args: host_call(*structs(w, *args)), sniff=host_sniff)


def odd_sources(rng, P=24):
    """(3, P, 2) points, (3, P) amounts and fields over the hand world's envs: on open and closed cells, on cell edges, outside,
    at NaN and far away; amounts 0, -1 and NaN among them; field indices -1 and 2 (G = 2) among them."""
    points = (rng.randint(-2, 18, (3, P, 2))*F(CELL/2)).astype(F)                     # half-cell steps: every other one on an edge
    points[:, 0], points[:, 1, 0] = np.nan, 3e10
    amounts = rng.choice(np.array([0, -1, np.nan, .5, 1, 3e-8, 100], F), (3, P))
    field = rng.randint(-1, 3, (3, P)).astype(np.int32)
    points[:, 2], amounts[:, 2], field[:, 2] = (.14, .01), 1., 0                      # ON the closed cell (0, 1) of env 0
    points[:, 3], amounts[:, 3], field[:, 3] = (.8, .7), 1., 1                        # on its isolated cell (5, 6)
    return points, amounts, field


def hand_world(G=2, cell=CELL):
    """The hand-made grid, beside it a 9 x 7 env of open cells elsewhere on the plane and an env without cells."""
    return world([((0, 0, 7, 6), hand()), ((-2, -1, 9, 7), np.ones((7, 9), bool)), ((0, 0, 0, 0), np.zeros((0, 0), bool))], G, cell)


def subnormals(w, run):
    """One deposit of 1.0 at rate 0.25, keep 0.5, floor 0, compared after 64, 128, 130, 140 and 150 sub-steps in all: by 130 and
    140 the rule's store holds values below the least normal number."""
    tiny = []
    for t, T in enumerate((64, 64, 2, 10, 10)):
        sources = dict(points=np.tile(np.array([.3, .15], F), (3, 1, 1)), amounts=np.ones((3, 1), F)) if t == 0 else {}
        tick(w, run, **sources, rate=.25, keep=.5, floor=0., T=T)
        tiny.append(int(((w.rule[0] > 0) & (w.rule[0] < np.finfo(F).tiny)).sum()))
    assert tiny[2] > 0 and tiny[3] > 0


def mixed_ticks(w, run, T=3):
    """Three ticks over the hand grid's two envs: odd sources, then reset with mask, then no sources at all; sniffed after each."""
    rng = np.random.RandomState(5)
    for t in range(3):
        points, amounts, field = odd_sources(rng)
        reset, mask = (None, None) if t == 0 else (np.array([[1, 0], [1, 1], [1, 1]], bool), np.array([[1, 1], [0, 1], [1, 1]], bool))
        before = w.V.copy()
        tick(w, run, **(dict(points=points, amounts=amounts, field=field) if t < 2 else {}), reset=reset, mask=mask, T=T)
        if t:                                                           # store (1, 0) was masked out: it kept its bits, reset or not
            at = w.G*int(w.starts[1])
            assert np.array_equal(bits(w.V[at:at + 63]), bits(before[at:at + 63])) and before[at:at + 63].any()
        sniff(w, run, points, field)
    return w


@pytest.mark.parametrize('T', [1, 3, 64])
def test_the_hand_made_grid_with_odd_sources_resets_and_masks_at_both_ends_of_T(T):
    w = mixed_ticks(hand_world(), host, T)
    assert w.scented[:2].max() > 0 and w.rule[0][1, 5, 6] > 0 and w.scented[2].tolist() == [0, 0]


ORDERS = [(0., [1., 3e-8, 3e-8]), (1., [2.**-24, 2.**-23])]


def ordered(run, resident, amounts):
    """(1 + 3e-8) + 3e-8 = 1 but (3e-8 + 3e-8) + 1 = 1.0000001; on a cell that holds 1: (1 + 2^-24) + 2^-23 = 1 + 2^-23 but
    (1 + 2^-23) + 2^-24 = 1 + 2^-22, by ties to even.  rate 0, keep 1: the cell shows the sum itself."""
    still = dict(rate=0., keep=1., floor=0., T=1)
    points = np.tile(np.array([.3, .15], F), (3, len(amounts), 1))                  # cell (1, 2)
    w = hand_world(G=1)
    if resident:
        tick(w, run, points=np.ascontiguousarray(points[:, :1]), amounts=np.full((3, 1), resident, F), **still)
    tick(w, run, points=points, amounts=np.tile(np.array(amounts, F), (3, 1)), **still)
    reverse = scent_rule(w.envs[0][0], CELL, hand(), np.full((1, 6, 7), resident, F)*hand(), points[0], amounts[::-1], None, 0., 1., 0., 1)[0]
    assert bits(reverse[0, 1, 2]) != bits(w.rule[0][0, 1, 2])             # (a condition on the inputs: the order shows)


@pytest.mark.parametrize('resident,amounts', ORDERS)
def test_two_and_three_sources_on_one_cell_add_in_ascending_order(resident, amounts):
    ordered(host, resident, amounts)


def test_the_floor_cuts_a_tail_to_exact_zero_and_a_coarser_cell_rounds_the_gradient():
    one = dict(points=np.tile(np.array([1., .4], F), (3, 1, 1)), amounts=np.ones((3, 1), F))        # cell (1, 3) at c = 0.3
    cut, whole = (tick(hand_world(G=1, cell=.3), host, **one, floor=floor, T=8) for floor in (1e-3, 0.))
    assert 0 < cut.scented[0, 0] < whole.scented[0, 0] and cut.V[cut.V > 0].min() >= F(1e-3)
    sniff(cut, host, (np.random.RandomState(1).rand(3, 40, 2)*2).astype(F))


def test_subnormal_values_after_130_140_and_150_substeps():
    subnormals(hand_world(G=1), host)


def test_the_global_path_with_its_workspace_at_odd_and_even_T():
    free = np.random.RandomState(2).rand(203, 202) > .3
    for T in (1, 2, 3):
        w = world([((-5, 7, 202, 203), free), ((0, 0, 9, 7), np.ones((7, 9), bool))], 1)
        assert w.max_framed > 40944
        points = (np.random.RandomState(T).rand(2, 65, 2)*F(1.)).astype(F) + F(1.)
        points[1] -= F(1.)
        tick(w, host, points=points, amounts=np.ones((2, 65), F), T=T)
        tick(w, host, T=T)
        sniff(w, host, points)
        assert w.scented.min() > 9


def test_mass_is_conserved_without_decay_and_floor():
    """keep = 1, floor = 0, no further deposit: the float64 sum of the store over 200 sub-steps, against a float64 statement of the
    same scheme written apart from the rule (flux over open neighbour pairs).  Measured: the binary32 store's sum deviates from
    the float64 scheme's by at most 3.5e-8 relative, after 200 sub-steps; the test holds four times that."""
    free = np.random.RandomState(7).rand(37, 40) > .25
    w = world([((0, 0, 40, 37), free)], 1)
    points = (np.random.RandomState(8).rand(1, 30, 2)*F(4.5)).astype(F)
    tick(w, host, points=points, amounts=np.full((1, 30), 2.5, F), keep=1., floor=0., T=1)
    x = w.rule[0][0].astype(np.float64)
    for _ in range(4):
        tick(w, host, keep=1., floor=0., T=50)
        for _ in range(50):
            flux = np.zeros_like(x)
            for axis in (0, 1):
                a, b = (np.moveaxis(v, axis, 0) for v in (x, free))
                d = np.where(b[1:] & b[:-1], a[1:] - a[:-1], 0.)*.2
                f = np.moveaxis(flux, axis, 0)
                f[:-1] += d
                f[1:] -= d
            x = x + flux
        print('relative deviation', abs(x.sum() - w.rule[0].sum(dtype=np.float64))/x.sum())
        assert abs(x.sum() - w.rule[0].sum(dtype=np.float64)) <= 4*3.5e-8*x.sum()
    assert x.sum() > 50


REFUSALS = dict(n_fields=0, n_sources=1025, points=None, amounts=None, rate=.26, keep=1.01, floor=float('inf'), substeps=0, values=None,
                peaks=None, scented=None)


@pytest.mark.parametrize('member,value', list(REFUSALS.items()) + [('n_sources', -1), ('rate', -.1), ('rate', float('nan')), ('keep', -.1),
                                                                  ('keep', float('nan')), ('floor', -1.), ('floor', float('nan')),
                                                                  ('substeps', 65), ('field', None), ('points', 4), ('workspace', 'values')])
def test_every_refusal(member, value):
    from megastep_amd import _lib
    w = hand_world()
    points, amounts, field = odd_sources(np.random.RandomState(0))
    grid, spec = structs(w, points, amounts, field, None, None, .2, .9, 0., 2)
    assert host_call(grid, spec) == 0
    setattr(spec, member, {4: points.ctypes.data + 4, 'values': spec.values}.get(value, value))
    assert host_call(grid, spec) == -1 and _lib.lib().ms_nav_scent(C.byref(grid), C.byref(spec), None) == -1, (member, value)


def test_a_grid_beyond_the_top_tier_needs_the_workspace_and_the_query_refuses_alike():
    from megastep_amd import _lib, cuda
    caps = (C.c_int*3)()
    assert _lib.lib().ms_host_nav_scent_capacity(caps) == 0 and tuple(caps) == cuda.SCENT_CAPACITY
    w = world([((0, 0, 202, 203), np.ones((203, 202), bool))], 1)
    grid, spec = structs(w, None, None, None, None, None, .2, .9, 0., 1)
    spec.workspace = None
    assert host_call(grid, spec) == -1
    points = np.zeros((1, 3, 2), F)
    for member, value in dict(n_points=0, n_fields=0, points=None, values=None, out=None).items():
        out = np.zeros((1, 3), F)
        query = _lib.MsNavScentQuery(3, points.ctypes.data, None, w.V.ctypes.data, 1, out.ctypes.data, None)
        assert host_call(grid, query) == 0
        setattr(query, member, value)
        assert host_call(grid, query) == -1 and _lib.lib().ms_nav_scent_query(C.byref(grid), C.byref(query), None) == -1, member
