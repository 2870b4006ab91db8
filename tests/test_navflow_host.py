"""Flow fields on the CPU: the host instantiations of the kernels' own per-cell functions (ms_host_nav_flows, ms_host_nav_flow_query:
csrc/kernels/navflow.h) held to EQUALITY with flow_rule (tests/flow_rule.py), as bytes - through both of the kernel's paths, the
framed codes and the stores (an env larger than the `max_framed` the grid declares takes the second)."""
import ctypes
import functools

import numpy as np
import pytest

from tests.flow_rule import FLOW_GOAL, flow_rule
from tests.test_navcost_host import cost_rule
from tests.test_navfield_host import CELL, F, INF, bits, nav_rule
from tests.test_navpath_host import NAN, cases, path_rule
from tests.test_navregion_host import _Host
from tests.test_navseed_host import seed_rule

# 13 rows of 12: a wall up column 5 with a doorway one cell wide (row 5), an L-shaped wall (row 8 and column 3), a pocket no path enters
FREE = np.ones((13, 12), bool)
FREE[:9, 5], FREE[5, 5], FREE[8, 3:6], FREE[8:11, 3], FREE[:2, 9], FREE[1, 9:] = False, True, False, False, False, False
GEOM = (-3, 2, 12, 13)
SEED = (11, 1)
GOAL = np.array(path_rule.centre(GEOM, CELL, 2, 9), F) + np.array([.03, -.02], F)      # inside a cell, off its centre
COST = (1 + 6*(np.indices(FREE.shape)[0] > 8)).astype(F)               # the rows past the L-shaped wall are dear


@functools.lru_cache(None)
def field(kind):
    """(world, table, cost or None), computed once: a single-goal, a seeded or a cost field of the hand-made plan; 'stale', the first
    with values overwritten after relaxation; 'plain' and 'oblique', the goal fields of two of test_navfield_host.plans."""
    if kind in ('plain', 'oblique'):
        return cases()[4*(kind == 'oblique')].world, cases()[4*(kind == 'oblique')].table, None
    seeds, rng = np.zeros(FREE.shape, bool), np.random.RandomState(4)
    seeds[SEED], seeds[2, 8], hit = True, True, FREE & (rng.rand(*FREE.shape) < .3)
    D = seed_rule.field(FREE, CELL, seeds) if kind == 'seeded' else cost_rule.field(FREE, CELL, seeds, COST) if kind == 'cost' else nav_rule.field(FREE, GEOM, CELL, GOAL)
    if kind == 'stale':
        D[hit], D[6, 8], D[7, 8] = rng.uniform(0, 3, hit.sum()).astype(F), NAN, -INF
    world = (GEOM, CELL, FREE, D, None if kind in ('seeded', 'cost') else GOAL)
    table = seed_rule.hops(world[:4]) if kind == 'seeded' else cost_rule.hops(world[:4], COST) if kind == 'cost' else path_rule.hops(world)
    return world, table, COST if kind == 'cost' else None


def host(world, L, points, cost=None, max_framed=None, store=None, envs=1, G=1, mask=None):
    """ms_host_nav_flows on `envs` copies of the world with G copies of its field each, then ms_host_nav_flow_query of `points` (P, 2)
    asked of field 0 of env 0 - on `store` where one is given: (targets, written over -7; way (P, 2); took (P,))."""
    from megastep_amd import _lib
    geom, cell, free, D, q = world
    h = _Host([geom]*envs, np.arange(envs + 1)*free.size, np.tile(free.reshape(-1), envs), cell, max_framed)
    values, goals = np.tile(D.reshape(-1), envs*G).astype(F), None if q is None else np.tile(np.array(q, F), (envs, G, 1))
    cost, mask = None if cost is None else np.tile(cost.reshape(-1), envs), None if mask is None else np.array(mask, np.uint8)
    ptr = lambda a: None if a is None else a.ctypes.data
    kind, out = (ptr(goals), ptr(cost), 0 if cost is None else 1), np.full(values.size, -7, np.int32)
    assert h.h.ms_host_nav_flows(ctypes.byref(h.grid), ctypes.byref(_lib.MsNavFlows(G, values.ctypes.data, *kind, L, ptr(mask), out.ctypes.data))) == 0
    asked, goal = np.zeros((envs, len(points), 2), F), np.zeros((envs, len(points)), np.int32)
    asked[0] = points
    way, took = np.full(asked.shape, F(-7), F), np.full(goal.shape, -7, np.int32)
    query = _lib.MsNavFlowQuery(len(points), asked.ctypes.data, goal.ctypes.data, values.ctypes.data, *kind, G, (out if store is None else store).ctypes.data,
                                way.ctypes.data, took.ctypes.data)
    assert h.h.ms_host_nav_flow_query(ctypes.byref(h.grid), ctypes.byref(query)) == 0
    return out, way[0], took[0]


def _points(world, rng, count):
    """`count` points within half a cell of free cells' centres."""
    geom, cell, free = world[:3]
    i, j = (a[rng.randint(0, free.sum(), count)] for a in np.nonzero(free))
    return (np.array([path_rule.centre(geom, cell, a, b) for a, b in zip(i, j)], F) + rng.uniform(-.5, .5, (count, 2))*cell).astype(F)


@pytest.mark.parametrize('kind,L,framed', [(kind, L, framed) for kind in ('goal', 'seeded', 'cost') for L in (1, 2, 16, 64) for framed in (True, False)]
                         + [(kind, 16, True) for kind in ('stale', 'plain', 'oblique')])
def test_the_host_instantiations_are_the_rule(kind, L, framed):
    world, table, cost = field(kind)
    live, q, plan = flow_rule.live(world), world[4], kind in ('plain', 'oblique')
    want = flow_rule.targets(world, table, L)
    points = _points(world, np.random.RandomState(L), 300 if plan else 80)
    points[:2] = [[NAN, 0.], [1e9, 1e9]]
    got, way, took = host(world, L, points, cost, None if framed else 16)  # (a grid that declares less than the env has: the stores' path)
    got = got.reshape(want.shape)
    ruled = [flow_rule.at(world, table, want, p) for p in points]
    answers = np.array([w for w, _ in ruled], F)
    assert np.array_equal(got, want), np.argwhere(got != want).tolist()
    assert np.array_equal(bits(way), bits(answers)) and took.tolist() == [t for _, t in ruled] and (took[:2] == -1).all() and (took == 1).sum() > 20
    # the store: -1 exactly off the live cells - walls, the pocket, a NaN; a seed, and a cell whose chain breaks at once, names itself
    named = live & ((table[0] == -1) | ((table[0] == 0) & (q is None)) | (L == 1))
    assert np.array_equal(got == -1, ~live) and (world[2] & ~live).any() and np.array_equal(got[named], np.flatnonzero(named))
    assert kind == 'stale' or (got[table[0] == 0] == FLOW_GOAL).all() == (got == FLOW_GOAL).any() == (q is not None and L >= 2)
    assert kind != 'stale' or (live & (table[0] == -1)).sum() >= 5
    if plan:                            # an answer is in the point's sight or its L = 2 waypoint, and finite exactly where the waypoint is
        floor, full = (np.array([path_rule.waypoint(world, p, k, table)[0] for p in points], F) for k in (2, 16))
        assert np.array_equal(np.isfinite(answers), np.isfinite(full)) and np.isfinite(answers).all(1).sum() > 150 and np.mean(took == 0) < .5
        for p, w, low in zip(points, answers, floor):
            assert not np.isfinite(w).all() or path_rule.sights(world, p, w[:1], w[1:])[0] or np.array_equal(bits(w), bits(low)), (p, w, low)


def test_a_masked_call_leaves_the_other_stores_alone():
    world, table, _ = field('seeded')
    got, _, _ = host(world, 16, np.zeros((1, 2), F), envs=2, G=2, mask=[[0, 1], [1, 0]])
    want, kept = flow_rule.targets(world, table, 16).reshape(-1), np.full(FREE.size, -7, np.int32)
    assert np.array_equal(got, np.concatenate([kept, want, want, kept]))


def test_bad_arguments_are_refused_before_anything_is_written_and_the_capacities_are_the_kernels():
    from megastep_amd import _lib, nav
    world, _, cost = field('cost')
    h = _Host([GEOM], [0, FREE.size], FREE)
    D, out, way = np.ascontiguousarray(world[3]), np.full(FREE.size, -7, np.int32), np.zeros((1, 1, 2), F)
    flows = dict(n_fields=1, fields=D.ctypes.data, goals=None, costs=cost.ctypes.data, n_costs=1, lookahead=16, mask=None, targets=out.ctypes.data)
    query = dict(n_points=1, points=way.ctypes.data, goal=None, fields=D.ctypes.data, goals=None, costs=None, n_costs=0, n_fields=1,
                 targets=out.ctypes.data, waypoints=way.ctypes.data, took=None)
    bad = {'flows': [dict(fields=None), dict(targets=None), dict(lookahead=0), dict(lookahead=65), dict(targets=D.ctypes.data)],
           'flow_query': [dict(points=None), dict(fields=None), dict(targets=None), dict(waypoints=None)]}
    for name, struct, good in (('flows', _lib.MsNavFlows, flows), ('flow_query', _lib.MsNavFlowQuery, query)):
        call = getattr(h.h, f'ms_host_nav_{name}')
        assert call(ctypes.byref(h.grid), ctypes.byref(struct(**good))) == 0 and call(ctypes.byref(h.grid), None) == call(None, None) == -1
        out[:] = -7
        for change in bad[name]:                                         # (-1: MS_EINVAL)
            assert call(ctypes.byref(h.grid), ctypes.byref(struct(**{**good, **change}))) == -1 and (out == -7).all(), change
    caps = (ctypes.c_int*3)()
    assert h.h.ms_host_nav_flow_capacity(caps) == 0 and tuple(caps) == nav.FLOW_CAPACITY == (16*1024, 64*1024, 160*1024)
