"""Projectiles on the CPU: ms_host_projectiles - projectile_kernel's own __host__ __device__ pieces, swept serially - held to fly_rule
in the whole store and every record, floats by their bits; every refusal; and the rule against float64 geometry written apart from it."""
import numpy as np
import pytest

from tests import projectile_rule as pr
from tests.percept_rule import plan_percepts
from tests.projectile_rule import F, KEYS, NAN, ROOM


def both(walls, agents, angles, store, ticks=1, **kw):
    """`ticks` calls in a row through the host statement and the rule, compared after each; the last rule result."""
    for _ in range(ticks):
        got, want = pr.host_fly(walls, pr.model(), agents, angles, store, **kw), pr.fly_rule(walls, pr.model(), agents, angles, store, **kw)
        pr.same(got, want, KEYS)
        store = {k: want[k] for k in pr.STORE}
    return want


@pytest.mark.parametrize('restitution', [1., .5])
@pytest.mark.parametrize('bounces', [0, 1, 3])
def test_the_box_room(bounces, restitution):
    """Straight at a wall; into a corner (two bounces in one tick, the second leg skipping the row of the first); fast enough to
    need all four legs; half a millimetre past the partition's end and half a millimetre onto it."""
    shots = [((.5, 2), (-8, 0)), ((.3, .35), (-6, -6)), ((2, 2), (10, 800)), ((3, .9995), (20, 0)), ((3, 1.0005), (20, 0))]
    store = pr.store(1, 2, 4, [(0, k, p, v, 64, bounces) for k, (p, v) in enumerate(shots)])
    agents, angles = np.array([[(1.5, 3.2), (7, .6)]], F), np.array([[30, -100]], F)
    first = both([ROOM], agents, angles, store, restitution=restitution)
    assert list(first['ended'][0, :5]) == {0: [2, 2, 2, 0, 2], 1: [0, 2, 2, 0, 0], 3: [0, 0, 2, 0, 0]}[bounces]
    assert list(first['bounces'][0, :3]) == [max(bounces - 1, 0), max(bounces - 2, 0), 0]
    both([ROOM], agents, angles, store, ticks=4, restitution=restitution)


@pytest.mark.parametrize('muzzle', [.25, .05])
def test_fire(muzzle):
    """Env 0: agent 0 with every slot full misfires, agents 1 and 3 fire in one tick, agent 2 is nowhere, agent 3 stands in front of
    agent 1 - whose shot starts inside its own outline at the small muzzle offset, flies out of it and strikes 3; slots 4 and 5 strike
    agent 0 from both sides; slot 7's timer reaches 0 in a tick in which it hits nothing. Env 1: reset with fire set."""
    store = pr.store(2, 4, 2, [(0, 0, (1, 3.5), (0, 0), 64, 0), (0, 1, (2, 3.5), (0, 0), 64, 0), (0, 2, (5, 3.5), (1, 0), 64, 0),
                               (0, 4, (.6, 1), (8, 0), 64, 0), (0, 5, (1.4, 1), (-8, 0), 64, 0), (0, 7, (6, .5), (3, 0), 1, 0),
                               (1, 5, (5, 3.5), (1, 0), 64, 2)])
    agents, angles = np.array([[(1, 1), (2, 2), (NAN, 1), (2.5, 2)]]*2, F), np.array([[0, 0, 0, 90]]*2, F)
    want = both([ROOM, ROOM], agents, angles, store, fire=np.ones((2, 4), np.uint8), reset=np.array([0, 1], np.uint8), muzzle=muzzle, life=5, bounces=1)
    assert list(want['misfires'][0]) == [1, 0, 0, 0] and not want['misfires'][1].any()
    assert want['struck'][0, 3] == 3 and want['ended'][0, 3] == 1 and list(want['hits'][0]) == [2, 0, 0, 1] and list(want['scored'][0]) == [0, 1, 2, 0]
    assert np.isfinite(want['positions'][0, 6]).all() and want['timers'][0, 6] == 4 and np.isnan(want['positions'][0, 4:6]).all()
    assert list(want['ended'][0, [4, 5, 7]]) == [1, 1, 3] and list(want['struck'][0, [4, 5, 7]]) == [0, 0, -1]
    assert np.isnan(want['positions'][1]).all() and not want['timers'][1].any() and not want['bounces'][1].any() and (want['ended'][1] == 4).all()


REFUSALS = [[(k, None)] for k in ('positions', 'velocities', 'owners', 'timers', 'bounces', 'agents', 'angles', 'model', 'walls', 'starts')] + \
    [[(k, lambda p: p + 4)] for k in ('positions', 'velocities', 'agents', 'model', 'walls')] + \
    [[(k, lambda p: p + 2)] for k in ('timers', 'owners', 'bounces', 'struck', 'hits', 'scored', 'angles')] + \
    [[('n_slots', 7)], [('n_slots', 34), ('per_agent', 17)], [('per_agent', 0)], [('n_slots', 65), ('per_agent', 1), ('n_agents', 65)], [('n_envs', 0)]] + \
    [[(k, v)] for k, vs in (('restitution', (-.1, 1.1, NAN)), ('speed', (0., np.inf)), ('muzzle', (0., NAN)), ('fps', (0., np.inf)), ('life', (0,)),
                            ('n_bounces', (-1,))) for v in vs]


@pytest.mark.parametrize('spoil', REFUSALS, ids=lambda s: '-'.join(k for k, _ in s))
def test_the_argument_check_refuses(spoil):
    args = ([ROOM], pr.model(), np.ones((1, 2, 2), F), np.zeros((1, 2), F), pr.store(1, 2, 4))
    pr.host_fly(*args, expect=-1, spoil=spoil)
    pr.host_fly(*args)


def _crossings(legs, walls):
    """In float64: which legs properly cross a wall, and which pass within 1e-4 m of a wall's end."""
    legs, walls = np.asarray(legs, np.float64)[:, None, :], np.asarray(walls, np.float64)[None]
    p, q, a, b = legs[..., 0:2], legs[..., 2:4], walls[..., 0:2], walls[..., 2:4]
    side = lambda o, d, x: (d[..., 0] - o[..., 0])*(x[..., 1] - o[..., 1]) - (d[..., 1] - o[..., 1])*(x[..., 0] - o[..., 0])
    cross = (side(p, q, a)*side(p, q, b) < 0) & (side(a, b, p)*side(a, b, q) < 0)
    d = q - p
    def near(e):
        t = np.clip(((e - p)*d).sum(-1)/np.maximum((d*d).sum(-1), 1e-30), 0, 1)
        return np.linalg.norm(p + t[..., None]*d - e, axis=-1) < 1e-4
    return cross.any(1), (near(a) | near(b)).any(1)


@pytest.mark.parametrize('n', [1, 4])
def test_no_leg_crosses_a_wall_in_float64(n):
    """Some 125 shots each on an axis-aligned and on an oblique plan, 16 ticks, up to three bounces, the host statement held to the rule
    at every tick: no leg flown through the air crosses a static wall; those within 1e-4 m of a wall's end are left out, under 1 %."""
    v = plan_percepts()
    walls, ends = [v.walls[n]], np.concatenate([v.walls[n][:, :2], v.walls[n][:, 2:]])
    store = pr.random_store(1, 12, 16, [ends.min(0)], [ends.max(0)], n)
    store['timers'] += 30
    agents, angles, legs = v.points[n][None, :12], np.linspace(-170, 170, 12, dtype=F)[None], []
    for _ in range(16):
        out = pr.fly_rule(walls, pr.model(), agents, angles, store, legs=legs)
        pr.same(pr.host_fly(walls, pr.model(), agents, angles, store), out, KEYS)
        store = {k: out[k] for k in pr.STORE}
    crossed, close = _crossings(legs, walls[0])
    print(f'plan {n}: {len(legs)} legs, {int(close.sum())} within 1e-4 m of an end, {int((crossed & ~close).sum())} crossings')
    assert len(legs) > 500 and close.mean() < .01
    assert not (crossed & ~close).any()
