"""The fan schedule (MsAgents.schedule: costs | order) at small, odd shapes, on the device.

1. The sort waves in front of every physics launch (physics.h, fan_sort_wave) against the numpy rule of tests/test_fan_order_host.py
   (order_rule): fan counts of 1 ... 8196, runs of length 0 and 1, fan counts that do not divide by 8, K = 1 at its edge, K = 2 and
   K = 3 with shares of unequal length; through every instantiation of physics_kernel, packed and not.
2. Where the table is served and where it is not: a call it does not serve leaves both rows as they are.
3. The four render instantiations that follow the order (render_kernel<.,.,1,0>), dynlight_kernel's queue, the first-sight books
   and the crosshair ids under orders that are NOT the identity, against the oracle - and the cost a wave leaves, which belongs to
   its fan whatever slot the wave had.

Every order handed to a render is a permutation of the launch's fans; sentinels and odd bit patterns go into the costs row, and
into the order row only in front of a physics step, which sorts it afresh."""
import time

import numpy as np
import pytest
import torch

from tests import util
from tests.test_fan_order_host import assert_order_follows_the_rule, klass, order_rule, runs, shares

pytestmark = pytest.mark.gpu

SENTINEL = -12345
INT_MIN, INT_MAX = -2**31, 2**31 - 1


def _h():
    from megastep_amd import _lib
    return _lib.lib()


def _rows(c):
    """(costs, order) as numpy arrays - a copy, after everything enqueued has run."""
    rows = c.agents._schedule.cpu().numpy()
    return rows[0].copy(), rows[1].copy()


def _set_rows(c, costs=None, order=None):
    """Writes a row (an array) or fills it (a number); None leaves it."""
    for row, x in zip(c.agents._schedule, (costs, order)):
        if x is None:
            continue
        if np.isscalar(x):
            row.fill_(int(x))
        else:
            row.copy_(torch.as_tensor(np.ascontiguousarray(x, dtype=np.int32), device=row.device))


# ------------------------------------------------------------------------------------------------------------------------
# 1. the sort against the rule
# ------------------------------------------------------------------------------------------------------------------------
# (n_envs, n_agents): fans, sort waves a run (K), the eight runs' lengths, and for K > 1 the shares of a run of each length.
# Written out, not derived: a change of physics.h's FAN_SORT_MAX (512) fails _assert_shape instead of moving the cases off their edges.
SHAPES = {
    (1, 1): (1, 1, [1, 0, 0, 0, 0, 0, 0, 0], {}),                      # runs of length 0 and 1: a sort wave without a fan reads costs[n_fans],
    (1, 3): (3, 1, [1, 1, 1, 0, 0, 0, 0, 0], {}),                      # which is order[0] - inside the table, thrown away
    (7, 1): (7, 1, [1]*7 + [0], {}),
    (2, 4): (8, 1, [1]*8, {}),
    (3, 3): (9, 1, [2] + [1]*7, {}),
    (13, 3): (39, 1, [5]*7 + [4], {}),
    (1, 64): (64, 1, [8]*8, {}),
    (4096, 1): (4096, 1, [512]*8, {}),                                 # K = 1 at its edge
    (4097, 1): (4097, 2, [513] + [512]*7, {513: [257, 256], 512: [256, 256]}),
    (1025, 4): (4100, 2, [513]*4 + [512]*4, {513: [257, 256], 512: [256, 256]}),
    (8193, 1): (8193, 3, [1025] + [1024]*7, {1025: [342, 342, 341], 1024: [342, 341, 341]}),
    (2049, 4): (8196, 3, [1025]*4 + [1024]*4, {1025: [342, 342, 341], 1024: [342, 341, 341]}),
}


def _assert_shape(shape):
    n_fans, K, lengths, split = SHAPES[shape]
    assert n_fans == shape[0]*shape[1]
    assert [length for _, length in runs(n_fans)] == lengths
    parts, k = shares(n_fans)
    assert k == K and len(parts) == 8*K
    for x, length in enumerate(lengths):
        assert [count for _, count, _ in parts[x*K:(x + 1)*K]] == split.get(length, [length]), (x, length)
    return n_fans, K, parts


_boxes = {}


def _box_world(n_envs, n_agents, res=16):
    """n_envs copies of toys.box(), wall grid and all: the sort needs a real physics launch, not an interesting room."""
    key = (n_envs, n_agents, res)
    if key not in _boxes:
        _boxes[key] = util.plan_world(n_envs, n_agents, res, 130, toy='box')[0]
        assert _boxes[key].scenery._wg is not None
    return _boxes[key]


def _moved_runs(costs):
    """Does the rule's order differ from the identity in every run of two fans or more?"""
    order = order_rule(costs)[0]
    return all((order[first:first + length] != np.arange(first, first + length)).any() for first, length in runs(len(costs)) if length >= 2)


def _spread_shares(costs):
    """More than 3 classes in every share of more than 8 fans?"""
    cls = klass(costs)
    return all(len(np.unique(cls[first:first + count])) > 3 for first, count, _ in shares(len(costs))[0] if count > 8)


def _searched(make, *conditions):
    """The first seed's costs that meet the conditions: they are asked of the rule alone, before anything runs on the device."""
    for seed in range(256):
        costs = make(np.random.RandomState(seed)).astype(np.int32)
        if all(ok(costs) for ok in conditions):
            return costs
    raise AssertionError('no seed below 256 gives costs that move every run')


def sort_cost_sets(n_fans):
    """name -> (costs, no two fans of a share tie). Every set but the constant ones moves every run of two fans or more, by the
    rule; the random ones hold more than 3 classes in every share of more than 8 fans."""
    parts, K = shares(n_fans)
    filled = [(first, length) for first, length in runs(n_fans) if length]
    sets = {}
    sets['random 0..79'] = (_searched(lambda rng: rng.randint(0, 80, n_fans), _moved_runs, _spread_shares), False)
    # (few classes: long chains of LDS atomics on one counter)
    sets['random 0..11'] = (_searched(lambda rng: rng.randint(0, 12, n_fans), _moved_runs, _spread_shares), False)
    sets['constant 5'] = (np.full(n_fans, 5, np.int32), False)
    sets['constant 64'] = (np.full(n_fans, 64, np.int32), False)

    def patterns(rng):
        # any 32 bits are a cost: half the fans hold some (class 63, all but never less), the others a class below it, and -1,
        # INT_MIN and INT_MAX stand where the draw puts them
        bits = rng.randint(0, 2**32, n_fans, dtype=np.uint64).astype(np.uint32).view(np.int32)
        costs = np.where(rng.rand(n_fans) < .5, bits, rng.randint(0, 63, n_fans).astype(np.int32))
        at = rng.permutation(n_fans)[:3]
        costs[at] = np.array([-1, INT_MIN, INT_MAX], np.int32)[:len(at)]
        return costs
    sets['bit patterns'] = (_searched(patterns, _moved_runs), False)
    assert n_fans < 3 or {-1, INT_MIN, INT_MAX} <= set(sets['bit patterns'][0].tolist())
    # the two classes at the top, 62 | 63 and beyond: fan_class' comparison
    sets['62 63 64 in turn'] = ((62 + np.arange(n_fans) % 3).astype(np.int32), False)
    assert _moved_runs(sets['62 63 64 in turn'][0])

    def slow_last(rng):
        costs = rng.randint(0, 12, n_fans)
        costs[filled[-1][0] + filled[-1][1] - 1] = 63                  # the last fan of the last run that has one
        return costs
    sets['one slow fan, the last of the last run'] = (_searched(slow_last, _moved_runs), False)

    def quick_first(rng):
        costs = rng.randint(1, 12, n_fans)
        costs[[first for first, _ in filled]] = 0                      # the first fan of every run: the one that ends up last
        return costs
    sets['one quick fan at the head of every run'] = (_searched(quick_first, _moved_runs), False)
    if max(count for _, count, _ in parts) <= 64:                      # no ties: the order is the rule's, fan for fan
        rising, mixed, rng = np.zeros(n_fans, np.int32), np.zeros(n_fans, np.int32), np.random.RandomState(n_fans)
        for first, count, _ in parts:
            rising[first:first + count] = np.arange(count)
            mixed[first:first + count] = rng.permutation(count)
        sets['rising within a share'] = (rising, True)
        sets['distinct, shuffled within a share'] = (mixed, True)
        assert _moved_runs(rising)
    return sets


@pytest.mark.parametrize('shape', list(SHAPES), ids=lambda s: f'{s[0]}x{s[1]}')
def test_the_sort_waves_write_the_rules_order(shape):
    from megastep_amd import cuda
    began = time.time()
    n_fans, K, parts = _assert_shape(shape)
    sets = sort_cost_sets(n_fans)
    c = _box_world(*shape)
    built = time.time()
    for name, (costs, exact) in sets.items():
        _set_rows(c, costs, SENTINEL)
        cuda.physics(c.scenery, c.agents)
        got_costs, got_order = _rows(c)
        assert (got_costs == costs).all(), f'{name}: the sort only reads the costs'
        assert_order_follows_the_rule(costs, got_order, exact=exact, what=f'{shape}, {name}')
    print(f'sort, {shape[0]} x {shape[1]} = {n_fans} fans, K = {K}, {len(sets)} cost sets: world {built - began:.2f} s, sorts {time.time() - built:.2f} s')


def _agent_state(c):
    a = c.agents
    return [t.clone() for t in (a.angles, a.positions, a.angvelocity, a.velocity)]


def _set_agent_state(c, state):
    a = c.agents
    for t, s in zip((a.angles, a.positions, a.angvelocity, a.velocity), state):
        t.copy_(s)


@pytest.mark.parametrize('pack', [1, 2, 4])
@pytest.mark.parametrize('instantiation', ['plain', 'movement', 'extras', 'movement and extras'])
def test_every_physics_instantiation_sorts_in_front_of_itself(instantiation, pack):
    """physics_kernel<MOVE, EXTRA, PACK>: 13 envs of 3 agents with a wall grid, one, two and four envs a wave - 13 divides by
    neither, and a physics wave's number is its block's less the sort waves'. The order row is the rule's; progress, the agents
    and the bookkeeping are, as bits, those of the same call with the schedule switched off."""
    from megastep_amd import cuda
    began = time.time()
    c = _box_world(13, 3)
    N, A, S = 13, 3, 5
    h = _h()
    assert h.ms_host_physics_pack(N, A, 1, pack) == pack
    rng = np.random.RandomState(7)
    c.agents.positions[:] = torch.as_tensor(rng.uniform(2., 5., (N, A, 2)).astype(np.float32), device=c.device)
    c.agents.angles[:] = torch.as_tensor(rng.uniform(-180, 180, (N, A)).astype(np.float32), device=c.device)
    util.random_velocities(c, rng, speed=3.)
    c.agents.velocity[::2] *= 15.                                        # (4.5 m a step in a 5 m room: these stop at a wall)
    start = _agent_state(c)
    costs = sort_cost_sets(N*A)['random 0..79'][0]
    gen = torch.Generator().manual_seed(5)
    table = torch.tensor([[0., 0., 0.], [.3, 0., 0.], [-.3, 0., 0.], [0., .3, 0.], [0., -.3, 0.], [0., 0., 40.], [0., 0., -40.]], device=c.device)
    actions = torch.randint(0, 7, (N, A), generator=gen).to(c.device)
    mask0 = (torch.rand((N, A), generator=gen) < .3).to(c.device)
    choices = torch.randint(0, S, (N, A), generator=gen).to(c.device)
    spawn_p = (2. + 2.*torch.rand((N, A, S, 2), generator=gen)).to(c.device)
    spawn_a = (360*torch.rand((N, A, S), generator=gen) - 180).to(c.device)
    ages0 = torch.randint(0, 3, (N, A), generator=gen, dtype=torch.int32).to(c.device)
    maxima0 = torch.full((N, A), 2, dtype=torch.int32, device=c.device)
    fresh = torch.randint(3, 9, (N, A), generator=gen, dtype=torch.int32).to(c.device)
    results = {}
    try:
        h.ms_debug_physics_pack(pack)
        for on in (1, 0):
            _set_agent_state(c, start)
            _set_rows(c, costs, SENTINEL)
            h.ms_debug_render_order(on)
            kw, books = {}, []
            if 'movement' in instantiation:
                kw['movement'] = (actions, table, .875)
            if 'extras' in instantiation:
                mask, ages, maxima, imu = mask0.clone(), ages0.clone(), maxima0.clone(), torch.full((N, A, 3), float('nan'), device=c.device)
                kw.update(respawn=dict(mask=mask, choices=choices, positions=spawn_p, angles=spawn_a), imu=(imu, 360., 10.),
                          lifespans=dict(lifespans=ages, max_lifespans=maxima, fresh=fresh))
                books = [mask, ages, maxima, imu]
            p = cuda.physics(c.scenery, c.agents, **kw)
            results[on] = ([p.progress.clone()] + _agent_state(c) + books, _rows(c))
    finally:
        h.ms_debug_render_order(1)
        h.ms_debug_physics_pack(0)
    (outs_on, (costs_on, order_on)), (outs_off, (costs_off, order_off)) = results[1], results[0]
    assert (costs_on == costs).all()
    assert_order_follows_the_rule(costs, order_on, what=f'{instantiation}, {pack} envs a wave')
    assert (costs_off == costs).all() and (order_off == SENTINEL).all(), 'switched off, the launch has no sort waves'
    names = ['progress', 'angles', 'positions', 'angvelocity', 'velocity', 'respawn mask', 'lifespans', 'max_lifespans', 'imu']
    for name, x, y in zip(names, outs_on, outs_off):
        util.assert_bits(x, y, name)
    progress = outs_on[0]
    assert bool((progress < 1).any()) and bool((progress == 1).any()), 'some agents stop, some do not'
    if 'extras' in instantiation:
        assert int(outs_on[5].sum()) > int(mask0.sum()) > 0, 'agents respawned by request, and more at the end of their lifespans'
        assert bool(torch.isfinite(outs_on[8]).all())
    print(f'physics_kernel, {instantiation}, {pack} envs a wave: {time.time() - began:.2f} s')


# ------------------------------------------------------------------------------------------------------------------------
# 2. who writes the table, and who leaves it alone
# ------------------------------------------------------------------------------------------------------------------------
COSTS_MARK, ORDER_MARK = -777, SENTINEL


def _untouched(c, what):
    costs, order = _rows(c)
    assert (costs == COSTS_MARK).all(), f'{what} wrote the costs row'
    assert (order == ORDER_MARK).all(), f'{what} wrote the order row'


def _calls(c):
    """The calls of the hot path, each from marked rows: (name, thunk)."""
    from megastep_amd import cuda
    return [('physics', lambda: cuda.physics(c.scenery, c.agents)),
            ('the colour render', lambda: cuda.render(c.scenery, c.agents)),
            ('the depth-only render', lambda: cuda.render(c.scenery, c.agents, fields=('distances',))),
            ('the pooled render', lambda: cuda.render(c.scenery, c.agents, fields=(), pooled=dict(subsample=1, max_depth=10.))),
            ('step_render', lambda: cuda.step_render(c.scenery, c.agents))]


@pytest.mark.parametrize('res', [65, 128])
def test_more_than_64_rays_an_agent_leave_the_table_alone(res):
    """schedule_serves: an agent of more than 64 rays is more than one wave; neither the physics launch nor any render touches the table."""
    began = time.time()
    c = _box_world(4, 2, res)
    util.random_velocities(c, np.random.RandomState(res), speed=3.)
    for name, call in _calls(c):
        _set_rows(c, COSTS_MARK, ORDER_MARK)
        call()
        _untouched(c, f'{name} at {res} rays')
    print(f'unserved, {res} rays: {time.time() - began:.2f} s')


def test_at_64_rays_the_same_calls_rewrite_the_table():
    """... so that the tests around this one cannot pass for want of a writer: physics rewrites the order row (and only reads the
    costs), a render of one-group waves the costs row (and only reads the order), the two-launch step both."""
    began = time.time()
    c = _box_world(4, 2, 64)
    util.random_velocities(c, np.random.RandomState(1), speed=3.)
    costs = sort_cost_sets(8)['random 0..79'][0]
    for name, call in _calls(c):
        if name == 'physics':
            _set_rows(c, costs, ORDER_MARK)
        elif name == 'step_render':
            _set_rows(c, COSTS_MARK, ORDER_MARK)
        else:
            _set_rows(c, COSTS_MARK, np.arange(8)[::-1])
        call()
        got_costs, got_order = _rows(c)
        if name == 'physics':
            assert (got_costs == costs).all()
            assert_order_follows_the_rule(costs, got_order, what='physics at 64 rays')
        elif name == 'step_render':
            assert not _h().ms_debug_last_step_fused(), 'two agents an env: two launches'
            assert (got_order == np.arange(8)).all(), 'the marks are one class: sorted, they stay in fan order'
            assert (got_costs != COSTS_MARK).all() and (got_costs >= 0).all(), 'the render behind the sort leaves every fan\'s cost'
        else:
            assert (got_order == np.arange(8)[::-1]).all(), f'{name} only reads the order'
            assert (got_costs != COSTS_MARK).all() and (got_costs >= 0).all(), f'{name} leaves every fan\'s cost'
            assert _h().ms_debug_last_render_groups() == 1
    print(f'served at 64 rays: {time.time() - began:.2f} s')


def test_switched_off_or_several_ray_groups_a_wave_leave_the_table_alone():
    """ms_debug_render_order(0): no call touches the table. ms_debug_ray_groups(2) at 64 rays - render_plan takes a pinned 2 or 4 at
    any resolution - is a launch of the wide instantiation, which takes no schedule (render_prepare: L.plan.ng == 1): the render
    leaves both rows alone (the physics launch, which cannot know the render behind it, still sorts)."""
    from megastep_amd import cuda
    began = time.time()
    c = _box_world(4, 2, 64)
    h = _h()
    try:
        h.ms_debug_render_order(0)
        for name, call in _calls(c):
            _set_rows(c, COSTS_MARK, ORDER_MARK)
            call()
            _untouched(c, f'{name}, switched off,')
        h.ms_debug_render_order(1)
        h.ms_debug_ray_groups(2)
        for name, call in _calls(c)[1:4]:
            _set_rows(c, COSTS_MARK, ORDER_MARK)
            call()
            assert h.ms_debug_last_render_groups() == 2
            _untouched(c, f'{name}, two ray groups a wave,')
    finally:
        h.ms_debug_render_order(1)
        h.ms_debug_ray_groups(0)
    _set_rows(c, 0, np.arange(8))
    print(f'switched off / two ray groups: {time.time() - began:.2f} s')


def test_the_one_launch_step_leaves_the_table_alone():
    """One agent an env, 64 rays: cuda.step_render is one launch (render_kernel<.,.,1,1>) - no physics launch to sort in, and the
    fused instantiations take no schedule."""
    from megastep_amd import cuda
    began = time.time()
    c = _box_world(7, 1, 64)
    util.random_velocities(c, np.random.RandomState(2), speed=3.)
    for kw in (dict(), dict(fields=('distances',)), dict(fields=(), pooled=dict(subsample=4, max_depth=10.))):
        _set_rows(c, COSTS_MARK, ORDER_MARK)
        cuda.step_render(c.scenery, c.agents, **kw)
        assert _h().ms_debug_last_step_fused()
        _untouched(c, f'the one-launch step {kw}')
    _set_rows(c, 0, np.arange(7))
    print(f'one-launch step: {time.time() - began:.2f} s')


def test_agents_without_a_table_step_and_render_the_same_bits():
    """Agents.SCHEDULE = False: MsAgents.schedule is NULL; every call succeeds and computes what the agents with a table do -
    whose order, by then, is not the identity."""
    from megastep_amd import cuda
    began = time.time()
    kept = cuda.Agents.SCHEDULE
    try:
        cuda.Agents.SCHEDULE = False
        bare = util.plan_world(13, 3, 64, 130, toy='box')[0]
    finally:
        cuda.Agents.SCHEDULE = kept
    assert bare.agents._schedule is None and bare.agents._struct.schedule is None and bare.agents._plain.schedule is None
    tabled = _box_world(13, 3, 64)
    start = _agent_state(tabled)
    _set_rows(tabled, 0, np.arange(39))
    rollouts = []
    for c in (tabled, bare):
        _set_agent_state(c, start)
        rng, out = np.random.RandomState(4), []
        for step in range(3):
            util.random_velocities(c, rng, speed=12. if step == 1 else 3.)
            p = cuda.physics(c.scenery, c.agents)
            r = cuda.render(c.scenery, c.agents)
            out.append([p.progress.clone()] + _agent_state(c) + [getattr(r, f).clone() for f in cuda.FIELDS] + [c.scenery.lines.vals.clone()])
        rollouts.append(out)
    for step, (xs, ys) in enumerate(zip(*rollouts)):
        for k, (x, y) in enumerate(zip(xs, ys)):
            util.assert_bits(x, y, f'step {step}, tensor {k}')
    costs, order = _rows(tabled)
    assert (order != np.arange(39)).any() and len(np.unique(klass(costs))) > 1, 'the agents with a table were following an order of their own'
    print(f'no table: {time.time() - began:.2f} s')


# ------------------------------------------------------------------------------------------------------------------------
# 3. the followers under orders that are not the identity
# ------------------------------------------------------------------------------------------------------------------------
MAX_DEPTH = 7.
# Which instantiation a request reaches (render_prepare / render_enqueue, csrc/host/render.h): colour = screen or pooled RGB wanted;
# no colour -> <1,0,1,0>; colour and not one per-ray plane -> <2,1,1,0>; colour with pooled outputs, books or some plane missing ->
# <1,1,1,0>; all five planes and nothing else -> <0,1,1,0>, and without a light grid (several agents an env) dynlight_kernel
# behind it, whose queue names the fans it has to light. All at one ray group a wave: ms_debug_last_render_groups() == 1.
COLOUR = {'colour', 'planes, pooled RGB-D and the crosshair', 'pooled RGB-D alone', 'books next to pooled RGB-D'}


def books_rule(scenery, want, epoch):
    """The first-sight books a render of fresh ones (stamps 0, counts 0) leaves, from the oracle's planes, in numpy (explorer.py:34-58;
    render.h, OUT_SEEN): the texel under a ray that hit is min(floor(w*loc), w - 1) of its line's w, in binary32, and takes its
    env's epoch; a ray that missed stamps the LAST texel of the scenery to the credit of the last env; an env's count is the number of
    its texels stamped. (stamp per texel, count per env), int32."""
    idx, loc = want['indices'], want['locations']
    n = lambda t: t.cpu().numpy()
    hit = idx >= 0
    line = n(scenery.lines.starts).astype(np.int64)[:, None, None] + np.maximum(idx, 0)
    w = n(scenery.textures.widths)[line].astype(np.float32)
    along = np.minimum(np.floor(w*np.where(hit, loc, np.float32(0))), w - 1).astype(np.int64)
    texel = n(scenery.textures.starts).astype(np.int64)[line] + along
    stamp = np.zeros(scenery.textures.vals.shape[0], np.int32)
    count = np.zeros(len(epoch), np.int32)
    for e in range(len(epoch)):
        seen = np.unique(texel[e][hit[e]])
        stamp[seen] = epoch[e]
        count[e] = len(seen)
    if (~hit).any() and len(stamp):
        if stamp[-1] != epoch[-1]:
            count[-1] += 1
        stamp[-1] = epoch[-1]
    return stamp, count


class _Followed:
    """A world of floorplans at rest, the oracle's render of it, and the orders its renders are handed."""

    def __init__(self, n_envs, n_agents, res, light_grid=True):
        from megastep_amd import cuda
        kept = cuda.Scenery.LIGHT_GRID
        try:
            cuda.Scenery.LIGHT_GRID = light_grid
            self.c = c = util.plan_world(n_envs, n_agents, res, 130)[0]
            lit = c.scenery._as_struct().lg_vals is not None
        finally:
            cuda.Scenery.LIGHT_GRID = kept
        assert lit == light_grid
        self.main = (n_envs, n_agents, res) == (13, 3, 64)
        self.n_fans, self.res, self.light_grid = n_envs*n_agents, res, light_grid
        self.sub = 4 if res % 4 == 0 else 1
        self.centre = res//self.sub >= 2
        n_model = c.scenery.model.shape[0]
        self.AF = n_agents*n_model
        self.agent_rows = (c.scenery.lines.starts.long()[:, None] + torch.arange(self.AF, device=c.device)[None]).flatten()
        # the order a physics step sorts from a render's own costs (nobody moves: the agents are at rest)
        cuda.render(c.scenery, c.agents)
        cuda.physics(c.scenery, c.agents)
        first_costs, sorted_order = _rows(c)
        assert_order_follows_the_rule(first_costs, sorted_order, what='the first render\'s costs, sorted')
        ref = util.OracleWorld(c)
        ref.pull_baked(c); ref.pull_agents(c)
        self.want = want = ref.render()
        self.want_lines = ref.scene.lines_vals.copy()
        idx = want['indices']
        self.on_agent = ((idx >= 0) & (idx < self.AF)).any(-1).reshape(-1)          # fans with a ray on an agent
        W = res//self.sub
        mid = idx.reshape(n_envs, n_agents, W, self.sub)[..., self.sub//2][..., [W//2 - 1, W//2]] if self.centre else None
        self.want_centre = np.where((mid >= 0) & (mid < self.AF), mid//n_model, -1).astype(np.int32) if self.centre else None
        self.want_rgb, self.want_depth = util.pooled_rule(want['screen'], want['distances'], c.agent_radius, MAX_DEPTH, self.sub)
        self.want_stamp, self.want_count = books_rule(c.scenery, want, 1 + np.arange(n_envs, dtype=np.int32))
        if self.main:
            assert self.on_agent.any() and not self.on_agent.all(), 'some fans have a ray on an agent, some have none'
            assert (sorted_order != np.arange(self.n_fans)).any()
        ident = np.arange(self.n_fans)
        back, mixed = ident.copy(), None
        for first, length in runs(self.n_fans):
            back[first:first + length] = back[first:first + length][::-1]
        for seed in range(64):                                           # (the first seed that moves something)
            rng, mixed = np.random.RandomState(seed), ident.copy()
            for first, length in runs(self.n_fans):
                mixed[first:first + length] = rng.permutation(mixed[first:first + length])
            if (mixed != ident).any():
                break
        self.orders = {'identity': ident, 'runs reversed': back, 'shuffled within runs': mixed,
                       'shuffled across runs': np.random.RandomState(2).permutation(self.n_fans), 'sorted by the last render\'s costs': sorted_order}
        for name, order in self.orders.items():
            assert sorted(order.tolist()) == ident.tolist(), name
            assert name in ('identity', 'sorted by the last render\'s costs') or (order != ident).any(), name
        pooled = dict(subsample=self.sub, max_depth=MAX_DEPTH)
        self.requests = {'colour': dict(), 'distances': dict(fields=('distances',))}
        if light_grid:
            self.requests.update({
                'indices, distances and pooled depth': dict(fields=('indices', 'distances'), pooled=dict(pooled, rgb=False, depth=True)),
                'planes, pooled RGB-D and the crosshair': dict(fields=cuda.FIELDS, pooled=dict(pooled, rgb=True, depth=True, centre=self.centre)),
                'pooled RGB-D alone': dict(fields=(), pooled=dict(pooled)),
                'books next to indices': dict(fields=('indices',), seen=True),
                'books next to pooled RGB-D': dict(fields=(), pooled=dict(pooled), seen=True)})
        self._identity = {}

    def run(self, name, order):
        """The request under the order, checked against the oracle: (costs row, the books' stamps and counts or None)."""
        from megastep_amd import cuda
        c, want = self.c, self.want
        kw = dict(self.requests[name])
        books = None
        if kw.pop('seen', False):
            books = (torch.zeros(c.scenery.textures.vals.shape[0], dtype=torch.int32, device=c.device),
                     1 + torch.arange(c.n_envs, dtype=torch.int32, device=c.device), torch.zeros(c.n_envs, dtype=torch.int32, device=c.device))
            kw['seen'] = books
        c.scenery.lines.vals[self.agent_rows] = 0.                      # (the draw step must happen under every order)
        _set_rows(c, SENTINEL, order)
        r = cuda.render(c.scenery, c.agents, **kw)
        assert _h().ms_debug_last_render_groups() == 1
        costs, order_after = _rows(c)
        assert (order_after == order).all(), f'{name}: a render only reads the order'
        assert (costs != SENTINEL).all(), f'{name}: fans {np.nonzero(costs == SENTINEL)[0][:8].tolist()} left no cost'
        util.assert_bits(c.scenery.lines.vals, self.want_lines, f'{name}: the drawn agents')
        fields = cuda.FIELDS if kw.get('fields') is None else kw['fields']
        for f in cuda.FIELDS:
            if f not in fields:
                assert getattr(r, f) is None, (name, f)
            elif f == 'indices':
                np.testing.assert_array_equal(r.indices.cpu().numpy(), want['indices'], err_msg=f'{name}: hit indices')
            else:
                util.assert_bits(getattr(r, f), want[f], f'{name}: {f}')
        pooled = kw.get('pooled')
        if pooled is not None:
            if pooled.get('rgb', True):
                util.assert_bits(r.obs_rgb, self.want_rgb, f'{name}: pooled rgb')
            if pooled.get('depth', True):
                util.assert_bits(r.obs_depth, self.want_depth, f'{name}: pooled depth')
            if pooled.get('centre', False):
                np.testing.assert_array_equal(r.obs_centre.cpu().numpy(), self.want_centre, err_msg=f'{name}: who is in the crosshair')
        if books is not None:
            stamp, count = books[0].cpu().numpy(), books[2].cpu().numpy()
            assert count.sum() > 0 and count.sum() == (stamp != 0).sum(), f'{name}: every texel stamped is counted once'
            np.testing.assert_array_equal(stamp, self.want_stamp, err_msg=f'{name}: the stamps of the texels under the oracle\'s rays')
            np.testing.assert_array_equal(count, self.want_count, err_msg=f'{name}: texels seen for the first time, per env')
            books = (stamp, count)
        return costs, books

    def identity(self, name):
        if name not in self._identity:
            self._identity[name] = self.run(name, self.orders['identity'])
        return self._identity[name]


WORLDS = {'13 x 3 x 64': (13, 3, 64, True), '13 x 3 x 64, no light grid': (13, 3, 64, False), '13 x 3 x 33': (13, 3, 33, True), '3 x 3 x 1': (3, 3, 1, True)}
ORDERS = ['identity', 'runs reversed', 'shuffled within runs', 'shuffled across runs', 'sorted by the last render\'s costs']
_followed = {}


@pytest.mark.parametrize('order', ORDERS)
@pytest.mark.parametrize('world', list(WORLDS))
def test_the_followers_compute_the_oracles_bits_under_any_order_and_leave_every_fan_its_own_cost(world, order):
    """Each request - through <0,1,1,0> (with and without dynlight_kernel behind it), <1,0,1,0>, <1,1,1,0>, <2,1,1,0>, with the
    first-sight books and the crosshair ids - under each order: the oracle's planes, drawn agents, pooled observations by
    util.pooled_rule; stamps and per-env counts those of books_rule on the oracle's planes and of the identity order; and the costs row, element for element, the one the
    same render leaves under the identity order - a cost is its fan's (fan_cost: windows, list length, rays redone, rays on agents,
    open lights - functions of the fan and the world), stored at n*A + a whatever slot the wave had."""
    began = time.time()
    if world not in _followed:
        _followed[world] = _Followed(*WORLDS[world])
    w = _followed[world]
    built = time.time()
    for name in w.requests:
        want_costs, want_books = w.identity(name)
        costs, books = w.run(name, w.orders[order])
        differ = np.nonzero(costs != want_costs)[0]
        assert not len(differ), f'{name}, {order}: fans {differ[:8].tolist()} report {costs[differ[:8]].tolist()}, under the identity order {want_costs[differ[:8]].tolist()}'
        if name in COLOUR:                                               # (the colourless instantiation lights nothing)
            assert (costs[w.on_agent] >= 10).all(), f'{name}, {order}: a fan with a ray on an agent costs 10 at least'
        if w.main:
            assert len(np.unique(klass(costs))) > 3, f'{name}: classes {np.unique(klass(costs)).tolist()}'
        if books is not None:
            assert (books[0] == want_books[0]).all() and (books[1] == want_books[1]).all(), f'{name}, {order}: the first-sight books'
    print(f'followers, {world}, {order}: world {built - began:.2f} s, {len(w.requests)} requests {time.time() - built:.2f} s; '
          f'classes of the colour render\'s costs {np.unique(klass(w.identity("colour")[0])).tolist()}')
