"""The step kernels' device-only text on the GPU: action tables at 1, 7, 21 (the last held in a register's lanes), 22
(the first read from memory) and 64 rows; actions far outside the table, among them one whose low 32 bits are a valid row; and the
LDS pair lists at their capacity - on tests/step_edges.py's constructions, whose counts tests/test_step_edges_host.py asserts on
the CPU and this module asserts again before each launch. Every comparison is of bits, against references the suite already has:
torch's own ops around a plain step, the chained step, the CPU oracle, the serial host statements."""
import numpy as np
import pytest
import torch

from tests import step_edges as se
from tests import util
from tests.rollout_rule import FIELDS, host_rollouts, rollout_rule, world_of
from tests.scenario_rule import host_scenarios
from tests.test_gpu_culls import _device
from tests.test_gpu_physics_pack import _restore, _state
from tests.test_gpu_rollouts import _same, stepped
from tests.test_gpu_scenarios import expanded, stepped as stepped_jointly
from tests.test_gpu_slide import ROLLED, _stepped as stepped_sliding, both
from tests.test_gpu_wallgrid import _world

pytestmark = pytest.mark.gpu

_KEPT = {}


def _kept(key, make):
    if key not in _KEPT:
        _KEPT[key] = make()
    return _KEPT[key]


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), device='cuda', dtype=dtype)


@pytest.fixture
def pack():
    from megastep_amd import _lib
    h = _lib.lib()
    yield h.ms_debug_physics_pack
    h.ms_debug_physics_pack(0)


@pytest.fixture
def scheme():
    from megastep_amd import _lib
    h = _lib.lib()
    yield h.ms_debug_rollout_scheme
    h.ms_debug_rollout_scheme(-1)


def _plan_world(n_envs, n_agents, seed):
    """A world of the suite's floorplans, kept for the module; every test starts it from the state it was made in."""
    def make():
        c, _ = _world(n_envs, n_agents, seed=seed, n_unique=min(n_envs, 6))
        util.random_velocities(c, np.random.RandomState(seed), speed=2., spin=30.)
        return c, _state(c)
    c, start = _kept(('plans', n_envs, n_agents, seed), make)
    _restore(c, start)
    return c


def _one_launch_world():
    def make():
        from tests.test_gpu_step_render import _world as render_world
        c, _ = render_world(48, 1, 64, 130., seed=3)
        util.random_velocities(c, np.random.RandomState(3), speed=2., spin=30.)
        return c, _state(c)
    c, start = _kept('one launch', make)
    _restore(c, start)
    return c


@pytest.fixture(scope='module', autouse=True)
def _the_models_thresholds():
    """The models in tests/step_edges.py count with the kernels' thresholds as the sources state them now (the CPU module asserts
    the same): a run of this module alone does not follow stale models."""
    c = se.constants()
    assert c == {k: getattr(se, k) for k in c}


def _mixed(progress, what=''):
    """Not vacuous: somebody ran into something, somebody did not."""
    assert (progress < 1).any() and (progress == 1).any(), what


# ---------------------------------------------------------------------------------------------------------------------
# A. table sizes
# ---------------------------------------------------------------------------------------------------------------------
def _moved_by_torch(c, actions, table, keep):
    """A copy of the agents with the movement modules' update done by torch's own ops (modules.py:57-66,106-118): the table
    gathered by the actions, turned into the global frame, blended with `keep` - through neither branch of the kernels' look-up."""
    from megastep_amd import cuda, modules
    a = c.agents
    ref = cuda.Agents(*(t.clone() for t in (a.angles, a.positions, a.angvelocity, a.velocity)))
    delta = table[actions]
    turned = modules.to_global_frame(ref.angles, delta[..., :2])
    if keep == 0:
        ref.angvelocity[:] = delta[..., 2]
        ref.velocity[:] = turned
    else:
        ref.angvelocity[:] = keep*ref.angvelocity + delta[..., 2]
        ref.velocity[:] = keep*ref.velocity + turned
    return ref


def _extras(c, seed):
    """respawn (after the step), lifespans and imu arguments of cuda.physics, twice over: the same values in tensors of their own."""
    N, A = c.agents.angles.shape
    rng = np.random.RandomState(seed)
    spots = c.agents.positions[:, :, None, :].repeat(1, 1, 3, 1).contiguous() + _dev(rng.uniform(-.02, .02, (N, A, 3, 2)).astype(np.float32))
    vals = dict(mask=rng.rand(N, A) < .3, choices=rng.randint(0, 3, (N, A)), ages=rng.randint(0, 5, (N, A)).astype(np.int32),
                fresh=rng.randint(5, 9, (N, A)).astype(np.int32))
    def one():
        respawn = dict(mask=_dev(vals['mask']), choices=_dev(vals['choices']), positions=spots, angles=torch.zeros((N, A, 3), device='cuda'), after=True)
        lifespans = dict(lifespans=_dev(vals['ages']), max_lifespans=torch.full((N, A), 4, dtype=torch.int32, device='cuda'), fresh=_dev(vals['fresh']))
        return dict(respawn=respawn, lifespans=lifespans, imu=(torch.full((N, A, 3), float('nan'), device='cuda'), 360., 10.))
    return one(), one()


def _physics_both(c, actions, table, keep, extras=None, slide=None, what=''):
    """cuda.physics(movement=) against the movement by torch's ops and a call without movement=: every output as bits. The agents
    are left as the call under test left them; returns its Physics."""
    from megastep_amd import cuda
    mine, theirs = extras if extras is not None else ({}, {})
    ref = _moved_by_torch(c, actions, table, keep)
    want = cuda.physics(c.scenery, ref, slide=slide, **theirs)
    got = cuda.physics(c.scenery, c.agents, movement=(actions, table, keep), slide=slide, **mine)
    for k in ('angles', 'positions', 'velocity', 'angvelocity'):
        util.assert_bits(getattr(c.agents, k), getattr(ref, k), what + k)
    for k in ('progress',) + (('slid', 'stopped') if slide else ()):
        util.assert_bits(getattr(got, k), getattr(want, k), what + k)
    if extras is not None:
        util.assert_bits(mine['imu'][0], theirs['imu'][0], what + 'imu')
        for k in ('lifespans', 'max_lifespans'):
            util.assert_bits(mine['lifespans'][k], theirs['lifespans'][k], what + k)
        assert torch.equal(mine['respawn']['mask'], theirs['respawn']['mask']) and mine['respawn']['mask'].any()
    return got


def _moves(T):
    return T > 1                                                         # (a table of the no-op alone: whoever moves is only slowing down)


@pytest.mark.parametrize('keep', [0., .875])
@pytest.mark.parametrize('T', se.TABLE_SIZES)
def test_physics_looks_actions_up_in_tables_of_every_size(pack, T, keep):
    """physics_kernel<MOVE>: plain, next to the envs' bookkeeping (EXTRA), one env a wave and four (PACK) on a gridded world, and
    with 66 agents an env - the last two read the table from memory whatever its size."""
    table = _dev(se.table(T))
    c = _plan_world(12, 3, 21)
    start = _state(c)
    actions = _dev(se.actions((12, 3), T, seed=T))
    assert set(se.must_rows(T)) <= set(actions.flatten().tolist())
    plain = _physics_both(c, actions, table, keep, what='plain: ').progress.clone()
    if _moves(T):
        _mixed(plain)
    _restore(c, start)
    _physics_both(c, actions, table, keep, extras=_extras(c, 5), what='with the books: ')
    for k in (1, 4):
        _restore(c, start)
        assert c.scenery._wg is not None
        pack(k)
        util.assert_bits(_physics_both(c, actions, table, keep, what=f'pack {k}: ').progress, plain, f'pack {k} against the plain call')
    pack(0)
    crowd = _plan_world(2, 66, 22)
    stood = crowd.agents.positions.clone()
    acts = _dev(se.actions((2, 66), T, seed=T + 1))
    acts[:, 64:] = _dev(np.array(se.must_rows(T))[[0, -1]])[None]        # (the agents beyond a wave's lanes take the first and the last row)
    p = _physics_both(crowd, acts, table, keep, what='66 agents: ')
    if _moves(T):
        _mixed(p.progress, '66 agents')
        assert (crowd.agents.positions[:, 64:] != stood[:, 64:]).any(), 'the agents beyond the first 64 moved'


@pytest.mark.parametrize('T', se.TABLE_SIZES)
def test_the_one_launch_step_and_the_sliding_step_look_actions_up_in_tables_of_every_size(T):
    from megastep_amd import _lib, cuda
    table = _dev(se.table(T))
    for keep in (0., .875):
        c = _one_launch_world()
        actions = _dev(se.actions((48, 1), T, seed=T))
        ref = _moved_by_torch(c, actions, table, keep)
        want = cuda.physics(c.scenery, ref)
        got, _ = cuda.step_render(c.scenery, c.agents, movement=(actions, table, keep))
        assert _lib.lib().ms_debug_last_step_fused() == 1
        for k in ('angles', 'positions', 'velocity', 'angvelocity'):
            util.assert_bits(getattr(c.agents, k), getattr(ref, k), f'one launch, keep {keep}: {k}')
        util.assert_bits(got.progress, want.progress, 'one launch: progress')
        if _moves(T):
            _mixed(got.progress)
        c = _plan_world(12, 3, 21)
        p = _physics_both(c, _dev(se.actions((12, 3), T, seed=T)), table, keep, slide=True, what=f'sliding, keep {keep}: ')
        if _moves(T):
            _mixed(p.progress)
            assert (p.slid > 0).any()


@pytest.mark.parametrize('T', se.TABLE_SIZES)
def test_rollouts_look_actions_up_in_tables_of_every_size(scheme, T):
    """rollout_kernel<0>, rollout_walls_kernel (pinned, and as the library picks it for eight candidates) and rollout_kernel<1>
    against the chained step."""
    from megastep_amd import cuda
    c = _plan_world(3, 2, 23)
    table = _dev(se.table(T))
    plans = _dev(se.actions((3, 2, 8, 3), T, seed=T))
    assert 8 <= se.ROLL_FEW
    want = stepped(c, plans, table, .875, others='rest')
    for which in (0, 1, -1):
        assert scheme(which) == 0
        got = cuda.rollouts(c.scenery, c.agents, plans, table, keep=.875, others='rest', trail=True)
        _same(got, want, f'scheme {which}: ')
    if T > 1:
        assert (got.stops > 0).any() and (got.stops == 0).any()
    sliding = cuda.rollouts(c.scenery, c.agents, plans, table, keep=.875, others='rest', trail=True, slide=True)
    want = stepped_sliding(c, plans, table, .875)
    for k in ROLLED:
        util.assert_bits(getattr(sliding, k), want[k], f'sliding: {k}')
    if T > 1:
        assert (sliding.slides > 0).any()


@pytest.mark.parametrize('T', se.TABLE_SIZES)
def test_scenarios_look_actions_up_in_tables_of_every_size(T):
    """scenario_kernel, joint and focal, against the chained step."""
    from megastep_amd import cuda
    c = _plan_world(3, 2, 23)
    table = _dev(se.table(T))
    joint = _dev(se.actions((3, 6, 2, 3), T, seed=T))
    got = cuda.scenarios(c.scenery, c.agents, joint, table, keep=.875, trail=True)
    _same(got, stepped_jointly(c, joint, table, .875), 'joint: ')
    if T > 1:
        assert (got.stops > 0).any() and (got.stops == 0).any()
    plans, base = _dev(se.actions((3, 2, 4, 3), T, seed=T + 1)), _dev(se.actions((3, 2, 3), T, seed=T + 2))
    focal = cuda.rollouts(c.scenery, c.agents, plans, table, keep=.875, others=base, trail=True)
    want = stepped_jointly(c, expanded(plans, base), table, .875)           # (N, A K, A, ..): agent f's plan k is scenario f K + k
    for k in FIELDS:
        rows = torch.stack([want[k][:, f*4:(f + 1)*4, f] for f in range(2)], 1)
        util.assert_bits(getattr(focal, k), rows.contiguous(), f'focal: {k}')
    if T > 1:
        assert (focal.stops > 0).any() and (focal.stops == 0).any()


@pytest.mark.parametrize('T', se.TABLE_SIZES)
def test_rolled_steps_at_heading_0_against_the_rule_over_the_oracle_and_the_host_statements(oracle, scheme, T):
    """One world heading along an axis under a table that never turns, where the host libm's sine is the device's
    (test_gpu_rollouts.test_against_the_rule_over_the_oracle): both rollout schemes and the scenarios, joint and focal."""
    from megastep_amd import cuda
    c = _plan_world(2, 2, 24)
    c.agents.angles[:] = 0.
    c.agents.angvelocity[:] = 0.
    table = se.straight(T)
    plans = se.actions((2, 2, 6, 3), T, seed=T)
    world = world_of(c)
    rule = rollout_rule(world, plans, table, .875, 'rest', c.agent_radius, c.fps)
    host = host_rollouts(world, plans, table, .875, 'rest', c.agent_radius, c.fps)
    for which in (0, 1):
        assert scheme(which) == 0
        got = cuda.rollouts(c.scenery, c.agents, _dev(plans), _dev(table), keep=.875, others='rest', trail=True)
        _same(got, rule, f'scheme {which} against the rule: ')
        _same(got, host, f'scheme {which} against the host statement: ')
    joint = se.actions((2, 5, 2, 3), T, seed=T + 1)
    _same(cuda.scenarios(c.scenery, c.agents, _dev(joint), _dev(table), keep=.875, trail=True),
          host_scenarios(world, joint, table, .875, c.agent_radius, c.fps), 'joint: ')
    base = se.actions((2, 2, 3), T, seed=T + 2)
    _same(cuda.rollouts(c.scenery, c.agents, _dev(plans), _dev(table), keep=.875, others=_dev(base), trail=True),
          host_scenarios(world, plans, table, .875, c.agent_radius, c.fps, base=base), 'focal: ')


# ---------------------------------------------------------------------------------------------------------------------
# B. actions outside the table
# ---------------------------------------------------------------------------------------------------------------------
def _three(shape, T, seed):
    """Actions with every wild value among valid rows; the clamped actions they must equal; what narrowing first would make of them."""
    return tuple(_dev(a) for a in se.wild(se.actions(shape, T, seed=seed), T))


def _outputs(c, p, slide=False):
    return _state(c) + [p.progress.clone()] + ([p.slid.clone(), p.stopped.clone()] if slide else [])


def _clamped(run, actions, what):
    """run(actions) -> a list of tensors: the wild actions give what the clamped ones give, bit for bit - and the narrowed ones do not."""
    wild, clamped, narrowed = actions
    got, want, other = run(wild), run(clamped), run(narrowed)
    for i, (x, y) in enumerate(zip(got, want)):
        util.assert_bits(x, y, f'{what}: output {i}')
    assert any(not util.same_bits(x, y).all() for x, y in zip(other, want)), f'{what}: narrowing first would have gone unseen'


@pytest.mark.parametrize('T', [21, 22])
def test_physics_clamps_wild_actions_in_64_bits(pack, T):
    """cuda.physics(movement=) plain, packed and with 66 agents; the one-launch step; the sliding step."""
    from megastep_amd import _lib, cuda
    table = _dev(se.table(T))

    def stepper(c, start, slide=None, fused=False):
        def run(actions):
            _restore(c, start)
            if fused:
                p, _ = cuda.step_render(c.scenery, c.agents, movement=(actions, table, .875))
                assert _lib.lib().ms_debug_last_step_fused() == 1
            else:
                p = cuda.physics(c.scenery, c.agents, movement=(actions, table, .875), slide=slide)
            return _outputs(c, p, bool(slide))
        return run

    c = _plan_world(12, 3, 21)
    start = _state(c)
    for k in (0, 1, 4):
        pack(k)
        _clamped(stepper(c, start), _three((12, 3), T, 1), f'pack {k}')
    pack(0)
    _clamped(stepper(c, start, slide=True), _three((12, 3), T, 2), 'sliding')
    crowd = _plan_world(2, 66, 22)
    wild = se.wild(se.actions((2, 66), T, seed=3), T)[0]
    wild[:, 64:] = [[2**32 + 3, -2**40], [2**63 - 1, T]]                  # (the agents beyond the first 64 take wild values too)
    clamped, narrowed = np.clip(wild, 0, T - 1), np.clip(wild.astype(np.int32), 0, T - 1).astype(np.int64)
    _clamped(stepper(crowd, _state(crowd)), tuple(_dev(a) for a in (wild, clamped, narrowed)), '66 agents')
    one = _one_launch_world()
    _clamped(stepper(one, _state(one), fused=True), _three((48, 1), T, 4), 'one launch')


@pytest.mark.parametrize('T', [21, 22])
def test_rollouts_and_scenarios_clamp_wild_actions_in_64_bits(scheme, T):
    from megastep_amd import cuda
    c = _plan_world(3, 2, 23)
    table = _dev(se.table(T))
    fields = lambda r, names=FIELDS: [getattr(r, k) for k in names]
    for which in (0, 1):
        assert scheme(which) == 0
        _clamped(lambda a: fields(cuda.rollouts(c.scenery, c.agents, a, table, keep=.875, others='rest', trail=True)),
                 _three((3, 2, 8, 3), T, 5), f'scheme {which}')
    assert scheme(-1) == 0
    _clamped(lambda a: fields(cuda.rollouts(c.scenery, c.agents, a, table, keep=.875, others='rest', trail=True, slide=True), ROLLED),
             _three((3, 2, 8, 3), T, 6), 'sliding')
    _clamped(lambda a: fields(cuda.scenarios(c.scenery, c.agents, a, table, keep=.875, trail=True)), _three((3, 6, 2, 3), T, 7), 'joint')
    # (the others' plans only show in an agent's results if it meets them: every env's two agents a step apart)
    c.agents.positions[:, 1] = c.agents.positions[:, 0] + _dev(np.float32([.25, .05]))
    base = _three((3, 2, 3), T, 8)
    _clamped(lambda a: fields(cuda.rollouts(c.scenery, c.agents, a, table, keep=.875, others=base[1], trail=True)),
             _three((3, 2, 4, 3), T, 9), "focal, the agents' own plans")
    # ... everybody at rest at heading 0 on the no-op, agent 1 a step from agent 0 on the side the last row drives it from: clamped,
    # the wild values of env 1 run it into agent 0, whose own results then show a stop; narrowed first they leave it standing
    last = se.table(T)[T - 1, :2]
    c.agents.angles[:] = 0.
    c.agents.velocity[:] = 0.
    c.agents.angvelocity[:] = 0.
    c.agents.positions[:, 1] = c.agents.positions[:, 0] - _dev(np.float32(.25)*last/np.hypot(*last))
    plans = torch.zeros((3, 2, 4, 3), dtype=torch.int64, device='cuda')
    _clamped(lambda b: fields(cuda.rollouts(c.scenery, c.agents, plans, table, keep=.875, others=b, trail=True)), base, "focal, the others' base plans")


# ---------------------------------------------------------------------------------------------------------------------
# C. the pair lists, counted
# ---------------------------------------------------------------------------------------------------------------------
def _rosette_world(ros, grid, n_envs=1):
    """`n_envs` copies of a rosette as a Core, every agent where the rosette has it, heading 0 - and the env's static rows the
    rosette's own, bit for bit: what the CPU module counted is what the kernels meet."""
    from megastep_amd import arrdict, core, cuda, scene
    rows = ros.rows.copy()
    poked = np.flatnonzero(~np.isfinite(rows).all(1))
    rows[poked] = np.nan_to_num(rows[poked], nan=6.)                     # (the builder takes no NaN: put in behind its back)
    A = len(ros.homes)
    geom = arrdict.arrdict(walls=rows.astype(float).reshape(-1, 2, 2), lights=np.array([[4., 5.]]), masks=np.ones((4, 4), np.int16), res=.2)
    np.random.seed(0)
    sc = scene.scenery([geom]*n_envs, A, device='cuda', random=np.random.RandomState(0), bake=False)
    AF = A*sc.model.shape[0]
    for n in range(n_envs):
        for l in poked:
            sc.lines.vals[int(sc.lines.starts[n]) + AF + int(l)] = _dev(ros.rows[l].reshape(2, 2))
    cuda.bake(sc, wall_grid=grid)
    assert (sc._wg is not None) == grid
    c = core.Core(sc, res=64, fov=130., fps=10)
    assert c.fps == se.FPS and np.float32(c.agent_radius) == np.float32(se.RADIUS)
    c.agents.positions[:] = _dev(ros.positions)[None]
    c.agents.angles[:] = 0.
    c.agents.angvelocity[:] = 0.
    for walls in world_of(c)['walls']:
        util.assert_bits(walls, ros.rows, 'the static rows')
    return c


def _head(c, ros, heading):
    c.agents.positions[:] = _dev(ros.positions)[None]
    c.agents.velocity[:] = _dev(ros.velocity(heading))[None]
    c.agents.angles[:] = 0.
    c.agents.angvelocity[:] = 0.


def _near_lists(c, tasks, n=0):
    """The near lists physics would walk for agents with these tasks in env n, read from the scenery's own wall grid: the device's
    cell (ms_test_cell_at), its header, the tier near_count picks. Returns (counts, the lists' rows); every agent is covered."""
    wg = c.scenery._wg
    geom = wg.geom[n].cpu().numpy().astype(np.float32)
    pts = np.stack([t[:2] for t in tasks]).astype(np.float32)
    index, inside = _device('cell_at', [np.tile(geom, (len(pts), 1)), np.full(len(pts), wg.cell, np.float32), pts], [torch.int32, torch.uint8])
    cells, rows = wg.cells.cpu().numpy().view(np.uint32).reshape(-1, 4), wg.near_rows.cpu().numpy().reshape(-1, 4)
    counts, lists = [], []
    for task, i, ok in zip(tasks, index, inside):
        reach = se.reach_of(task)
        assert ok and reach <= np.float32(wg.reach)
        hdr = cells[int(wg.starts[n]) + int(i)]
        count = int(hdr[3] & 0xffff) if reach <= np.float32(wg.reach_lo) else int(hdr[3] >> 16)
        counts.append(count)
        lists.append(rows[int(hdr[2]):int(hdr[2]) + count])
    return counts, lists


def _slid(steps, what):
    """The sliding steps of a world's headings ran their passes 1 and 2: somebody slid along what it met, somebody stopped dead."""
    assert any(bool((p.slid > 0).any()) for p in steps) and any(bool((p.stopped > 0).any()) for p in steps), what


def _against_the_oracle(c, what):
    from megastep_amd import cuda
    ref = util.OracleWorld(c)
    p = cuda.physics(c.scenery, c.agents)
    util.assert_physics_bits(c, p, *ref.physics())
    return p.progress.clone()


@pytest.mark.parametrize('name', list(se.SWEEPS))
def test_the_sweeps_list_at_its_capacity(name):
    """physics_kernel without a grid: the `few` and the `!few` sweep, lists filled to their last slot, flushed one pair later,
    more than one round of rows, an odd row among a few agents' - against the oracle, which meets every wall; and the sliding
    step over the same rows against its host statement."""
    ros, spec = se.sweep(name)
    c = _kept(('sweep', name), lambda: _rosette_world(ros, False))
    seen, slid = [], []
    for heading in se.HEADINGS:
        se.check_sweep(name, heading)
        _head(c, ros, heading)
        seen.append(_against_the_oracle(c, f'{name} at {heading}'))
        _head(c, ros, heading)
        slid.append(both(c, what=f'sliding, {name} at {heading}: '))
    _mixed(torch.stack(seen), name)
    _slid(slid, name)


@pytest.mark.parametrize('name', list(se.GRIDDED))
def test_the_deals_list_at_its_capacity(name):
    """physics_kernel and physics_slide_kernel with a grid: 64 pairs (one each), 65 (the cull first), the list filled to its last
    slot, and a flush mid-deal - P and the pairs kept window by window read from the scenery's own grid before each launch."""
    ros, spec = se.gridded(name)
    c = _kept(('gridded', name), lambda: _rosette_world(ros, True))
    seen, slid = [], []
    for heading in se.HEADINGS:
        counts, lists = _near_lists(c, ros.tasks(heading))
        se.check_gridded(name, counts, lists, heading)
        _head(c, ros, heading)
        seen.append(_against_the_oracle(c, f'{name} at {heading}'))
        _head(c, ros, heading)
        slid.append(both(c, what=f'sliding, {name} at {heading}: '))
    _mixed(torch.stack(seen), name)
    _slid(slid, name)


def test_packed_waves_deal_covered_envs_beside_one_that_is_not(pack):
    """PACK: five envs two to a wave - the last wave holds one (E < pack_envs) - of four agents and twenty ring walls each, 80
    pairs an env; env 1's first agent stands outside the grid, so its env meets all its rows while env 0's pairs are dealt."""
    ros = se.Rosette('r'*20 + 'f'*4, [0]*4)
    c = _kept('packed', lambda: _rosette_world(ros, True, n_envs=5))
    seen, slid = [], []
    for heading in se.HEADINGS:
        _head(c, ros, heading)
        c.agents.positions[1, 0] = _dev(np.float32([-30., 2.]))
        tasks = ros.tasks(heading)
        for n in (0, 4):
            counts, lists = _near_lists(c, tasks, n)
            assert counts == [20]*4 and all(not se.beyond(t, row) for t, rows in zip(tasks, lists) for row in rows)
        _, inside = _device('cell_at', [c.scenery._wg.geom[1:2].cpu().numpy().astype(np.float32), np.float32([c.scenery._wg.cell]),
                                        np.float32([[-30., 2.]])], [torch.int32, torch.uint8])
        assert not inside[0]
        start = _state(c)
        pack(2)
        seen.append(_against_the_oracle(c, f'packed at {heading}'))
        _restore(c, start)
        pack(1)
        util.assert_bits(_against_the_oracle(c, f'alone at {heading}'), seen[-1])
        _restore(c, start)
        slid.append(both(c, what=f'sliding, packed world at {heading}: '))
    assert torch.stack(seen)[:, 1, 0].eq(1).all()                        # (the agent outside meets nothing)
    _mixed(torch.stack(seen)[:, [0, 2, 3, 4]])
    _slid(slid, 'the packed world')


@pytest.mark.parametrize('grid', [False, True], ids=['nowallgrid', 'wallgrid'])
@pytest.mark.parametrize('name', list(se.ROLLED))
def test_the_rollouts_list_at_its_capacity(scheme, name, grid):
    """rollout_walls_kernel: the list's lengths behind every window of step 0, counted (with a grid: over the near lists read from
    it); its bits against rollout_kernel's and against ms_host_rollouts."""
    from megastep_amd import cuda
    ros, spec = se.rolled(name)
    c = _kept(('rolled', name, grid), lambda: _rosette_world(ros, grid))
    _head(c, ros, 0.)
    c.agents.velocity[:] = 0.
    table, plans = se.straight(), se.rolled_plans(name)
    lists = None
    if grid:
        tasks = [se.task_of(ros.positions[0], table[plans[k, 0]][:2]) for k in range(spec['K'])]
        lists = _near_lists(c, tasks)[1]
    se.check_rolled(name, lists)
    got = []
    for which in (1, 0):
        assert scheme(which) == 0
        got.append(cuda.rollouts(c.scenery, c.agents, _dev(plans), _dev(table), keep=0., trail=True))
    _same(got[0], got[1], 'a lane a wall against a lane a candidate: ')
    _same(got[0], host_rollouts(world_of(c), plans, table, 0., None, c.agent_radius, c.fps), 'against the host statement: ')
    assert (got[0].stops > 0).any() and (got[0].stops == 0).any()


def test_lanes_walk_near_lists_of_0_1_3_4_and_5_rows_beside_one_no_list_covers(scheme):
    """walk_rows (rollout_kernel, scenario_kernel): ROLL_AHEAD = 4 rows in flight - lists shorter, as long and longer, and a lane
    outside the grid that walks every row, among the lanes of one wave."""
    from megastep_amd import arrdict, core, cuda, scene
    rows, spots = se.spots_check()

    def make():
        geom = arrdict.arrdict(walls=rows.astype(float).reshape(-1, 2, 2), lights=np.array([[4., 5.]]), masks=np.ones((4, 4), np.int16), res=.2)
        np.random.seed(0)
        sc = scene.scenery([geom], len(spots), device='cuda', random=np.random.RandomState(0), bake=False)
        cuda.bake(sc, wall_grid=True)
        return core.Core(sc, res=64, fov=130., fps=10)
    c = _kept('spots', make)
    c.agents.positions[:] = _dev(spots)[None]
    c.agents.angles[:] = 0.
    c.agents.velocity[:] = 0.
    c.agents.angvelocity[:] = 0.
    table = se.straight()
    util.assert_bits(world_of(c)['walls'][0], rows, 'the static rows')
    for row in table[1:]:                                                # (whichever row a lane takes at step 0)
        counts, _ = _near_lists(c, [se.task_of(p, row[:2]) for p in spots[:-1]])
        assert tuple(counts) == se.SPOT_ROWS[:-1] and se.ROLL_AHEAD == 4
    _, inside = _device('cell_at', [c.scenery._wg.geom[:1].cpu().numpy().astype(np.float32), np.float32([c.scenery._wg.cell]), spots[-1:]],
                        [torch.int32, torch.uint8])
    assert not inside[0]
    world = world_of(c)
    plans = 1 + se.actions((1, len(spots), 8, 3), 6, seed=1)
    assert scheme(0) == 0
    got = cuda.rollouts(c.scenery, c.agents, _dev(plans), _dev(table), keep=0., trail=True)
    _same(got, host_rollouts(world, plans, table, 0., None, c.agent_radius, c.fps), 'rollouts: ')
    assert (got.stops[0, 1:5] > 0).any() and (got.stops == 0).any()
    joint = 1 + se.actions((1, 4, len(spots), 3), 6, seed=2)                # (24 lanes of one wave: every length side by side)
    got = cuda.scenarios(c.scenery, c.agents, _dev(joint), _dev(table), keep=0., trail=True)
    _same(got, host_scenarios(world, joint, table, 0., c.agent_radius, c.fps), 'scenarios: ')
    assert (got.stops[0, :, 1:5] > 0).any() and (got.stops == 0).any()
