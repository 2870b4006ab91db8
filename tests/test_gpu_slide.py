"""Sliding contacts on the GPU: physics_slide_kernel against ms_host_slide - the serial host statement of the same
per-agent functions, which tests/test_slide_host.py holds to the rule over the oracle - as bits in positions, angles, velocities,
progress, slid, stopped and the IMU reading; with and without a wall grid; at one, four, five and 64 agents an env; next to the
environment's bookkeeping; the invariants that tie it to cuda.physics; and the call's plumbing."""
import ctypes as C
import numpy as np
import pytest
import torch

from tests import util
from tests.rollout_rule import world_of
from tests.slide_rule import FIELDS, STATE, host_slide
from tests.test_gpu_wallgrid import _world
from tests.test_gpu_physics_pack import _restore, _state

pytestmark = pytest.mark.gpu

# the movement modules' actions at 3 m/s without a turn (row 0: the no-op); row 5 takes 2 m a step - farther than the wall grid's
# lists reach; row 6 crawls at 6e-7 m a step, where project()'s "+ 1e-6" stretches the reach to metres
TABLE = [[0, 0, 0], [0, 3, 0], [0, -3, 0], [3, 0, 0], [-3, 0, 0], [0, 20, 0], [0, 6e-6, 0]]


def _host(t):
    return None if t is None else np.ascontiguousarray(t.detach().cpu().numpy())


def _extras(respawn, lifespans, imu):
    """The MsStepExtras of ms_host_slide over host copies of cuda.physics' respawn / lifespans / imu arguments, and the copies."""
    from megastep_amd import _lib
    if respawn is None and lifespans is None and imu is None:
        return None, {}
    x = _lib.MsStepExtras(imu_ang_scale=1., imu_speed_scale=1.)
    held = {}
    if respawn is not None:
        held.update(mask=_host(respawn['mask']).astype(np.uint8), choices=_host(respawn['choices']), positions=_host(respawn['positions']),
                    angles=_host(respawn['angles']))
        x.respawn_mask, x.respawn_choice = held['mask'].ctypes.data, held['choices'].ctypes.data
        x.spawn_positions, x.spawn_angles, x.n_spawns = held['positions'].ctypes.data, held['angles'].ctypes.data, held['positions'].shape[2]
        x.respawn_after = int(bool(respawn.get('after', False)))
    if lifespans is not None:
        held.update({k: _host(lifespans[k]) for k in ('lifespans', 'max_lifespans', 'fresh')})
        x.lifespans, x.max_lifespans, x.fresh_max = (held[k].ctypes.data for k in ('lifespans', 'max_lifespans', 'fresh'))
    if imu is not None:
        held['imu'] = np.full(tuple(imu[0].shape), np.nan, np.float32)
        x.imu, x.imu_ang_scale, x.imu_speed_scale = held['imu'].ctypes.data, float(imu[1]), float(imu[2])
    return x, held


def both(c, bounce=.05, movement=None, respawn=None, lifespans=None, imu=None, what=''):
    """One sliding step on the device and by ms_host_slide from the same state, equal as bits in every output - and `progress`
    equal to cuda.physics' on the same state. The agents are left where the sliding step put them; returns its Physics."""
    from megastep_amd import cuda
    start = _state(c)
    plain = cuda.physics(c.scenery, c.agents, movement=movement).progress.clone() if respawn is None and lifespans is None else None
    _restore(c, start)
    world = world_of(c)
    extras, held = _extras(respawn, lifespans, imu)
    mv = None if movement is None else (_host(movement[0]), _host(movement[1]), movement[2])
    want = host_slide(world, c.agent_radius, c.fps, bounce, mv, extras)
    got = cuda.physics(c.scenery, c.agents, movement=movement, respawn=respawn, lifespans=lifespans, imu=imu, slide=dict(bounce=bounce))
    a = c.agents
    for k, t in zip(FIELDS, (a.positions, a.angles, a.velocity, a.angvelocity, got.progress, got.slid, got.stopped)):
        util.assert_bits(t, want[k], what + k)
    if plain is not None:
        util.assert_bits(got.progress, plain, what + 'progress against cuda.physics')
    if imu is not None:
        util.assert_bits(imu[0], held['imu'], what + 'imu')
    if lifespans is not None:
        for k in ('lifespans', 'max_lifespans'):
            util.assert_bits(lifespans[k], held[k], what + k)
        util.assert_bits(respawn['mask'].to(torch.uint8), held['mask'], what + 'mask')
    return got


def _odd_poses(c, rng, speed=3.):
    """Velocities for everyone; env 1's first agent outside its grid (next to covered ones), env 2's faster than the lists reach,
    env 0's last agent crawling, and a NaN pose in the last env."""
    util.random_velocities(c, rng, speed=speed)
    pos, vel = c.agents.positions.clone(), c.agents.velocity.clone()
    N = pos.shape[0]
    if N > 1:
        pos[1, 0] = torch.tensor([-30., 2.])
    if N > 2:
        vel[2, 0] *= 20.
        pos[N - 1, -1] = float('nan')
    vel[0, -1] *= 1e-7
    c.agents.positions[:] = pos
    c.agents.velocity[:] = vel


def _custom(rows, grid, position):
    """One env of hand-made walls ((W, 2, 2)), one agent at `position` heading 0, with or without a wall grid."""
    from megastep_amd import arrdict, core, cuda, scene
    geom = arrdict.arrdict(walls=np.asarray(rows, float), lights=np.array([[4., 5.]]), masks=np.ones((4, 4), np.int16), res=.2)
    np.random.seed(0)
    scenery = scene.scenery([geom], 1, device='cuda', random=np.random.RandomState(0), bake=False)
    cuda.bake(scenery, wall_grid=grid)
    c = core.Core(scenery, res=64, fov=130., fps=10)
    assert (scenery._wg is not None) == grid
    c.agents.positions[0, 0] = torch.tensor(position, device='cuda')
    c.agents.angles[:] = 0.
    return c


def _mixed(p):
    """A step worth holding: some agents unblocked, some slid, some stopped dead."""
    blocked = p.progress < 1
    assert blocked.any() and (~blocked).any() and (p.slid > 0).any(), (int(blocked.sum()), int((p.slid > 0).sum()))


@pytest.mark.parametrize('grid', [True, False], ids=['wallgrid', 'nowallgrid'])
@pytest.mark.parametrize('n_envs,n_agents', [(37, 1), (9, 4), (3, 5), (2, 64)])
def test_the_kernel_is_the_host_statement_on_plans(n_envs, n_agents, grid):
    """(3, 5): beyond PHYS_FEW; five agents' near lists - a dozen rows or two each - and 64 agents' are more than 64 (row, agent)
    pairs an env: the cull-first, compact-in-LDS path (how many pairs, and the list at its capacity, are counted in
    tests/test_gpu_step_edges.py::test_the_deals_list_at_its_capacity). Three steps on: the second from the state the first left."""
    c, _ = _world(n_envs, n_agents, seed=4 + n_agents, n_unique=min(n_envs, 6), grid=grid)
    assert (c.scenery._wg is not None) == grid
    rng = np.random.RandomState(5)
    _odd_poses(c, rng)
    if n_agents > 1:
        c.agents.positions[0, 1] = c.agents.positions[0, 0] + torch.tensor([.25, .05], device='cuda')     # a pair a step apart
    p = both(c, what='step 0: ')
    _mixed(p)
    assert (p.stopped > 0).any()
    for step in (1, 2):
        util.random_velocities(c, rng, speed=2.)
        both(c, bounce=(0., 1.)[step - 1], what=f'step {step}: ')


def test_one_box_with_64_agents():
    c, _ = util.plan_world(1, 64, 64, 130., seed=3, toy='box')
    rng = np.random.RandomState(6)
    for step in range(3):
        util.random_velocities(c, rng, speed=4.)
        p = both(c, what=f'step {step}: ')
    _mixed(p)


def test_equal_values_with_different_normals_and_a_row_listed_twice():
    """The symmetric notch of tests/test_slide_host.py met head-on, with and without a wall grid, its rows in either order and one
    of them twice: equal x1 from two rows with mirror-image normals - the least key wins on every path, in any lane order."""
    outs = []
    notch = [[[0, 2], [-2, 4]], [[0, 2], [2, 4]]]
    frame = [[[-3, 0], [3, 0]], [[3, 0], [3, 6]], [[3, 6], [-3, 6]], [[-3, 6], [-3, 0]]]
    for rows in (notch + frame, notch[::-1] + frame, notch + frame + notch[:1]):
        for grid in (True, False):
            c = _custom(np.array(rows, float) + 4., grid, [4., 7.])
            c.agents.velocity[0, 0] = torch.tensor([0., -9.], device='cuda')
            if not outs:                                                 # (the tie, by the oracle's own test)
                from tests.slide_rule import _cs
                u = (np.float32(0), np.float32(np.float32(-9.)/np.float32(c.fps)))
                walls = world_of(c)['walls'][0]
                x = [_cs(np.float32([4., 7.]), u, walls[i], np.float32(c.agent_radius)) for i in (0, 1)]
                assert x[0] == x[1] < 1
            p = both(c)
            assert p.progress[0, 0] < 1
            outs.append([t.clone() for t in _state(c)] + [p.progress, p.slid, p.stopped])
    for o in outs[1:]:
        for x, y in zip(o, outs[0]):
            util.assert_bits(x, y)


@pytest.mark.parametrize('heading', [0., 90., 180.])
@pytest.mark.parametrize('keep', [0., .875])
def test_movement_at_headings_where_the_sine_is_exact(heading, keep):
    """The movement prologue and the IMU reading use the host libm's sine and cosine on the one side and the device's on the
    other: the agents head along an axis, where both are exact, and no action turns them."""
    c, _ = _world(9, 4, seed=8, n_unique=5)
    rng = np.random.RandomState(9)
    util.random_velocities(c, rng, speed=2., spin=0.)
    c.agents.angles[:] = heading
    actions = torch.as_tensor(rng.randint(-1, 9, (9, 4)), device='cuda')          # (out of the table at either end: clamped)
    table = torch.tensor(TABLE, dtype=torch.float32, device='cuda')
    imu = (torch.zeros((9, 4, 3), device='cuda'), 360., 10.)
    p = both(c, movement=(actions, table, keep), imu=imu)
    _mixed(p)


@pytest.mark.parametrize('after', [False, True])
def test_next_to_respawns_lifespans_and_the_imu(after):
    N, A, S = 9, 4, 3
    c, geoms = _world(N, A, seed=10, n_unique=5)
    rng = np.random.RandomState(11)
    _odd_poses(c, rng)
    c.agents.angles[:] = 0.
    c.agents.angvelocity[:] = 0.
    dev = 'cuda'
    spots = c.agents.positions[:, :, None, :].repeat(1, 1, S, 1).contiguous()
    spots += torch.as_tensor(rng.uniform(-.02, .02, (N, A, S, 2)).astype(np.float32), device=dev)
    respawn = dict(mask=torch.as_tensor(rng.rand(N, A) < .3, device=dev), choices=torch.as_tensor(rng.randint(-1, S + 1, (N, A)), device=dev),
                   positions=spots, angles=torch.zeros((N, A, S), device=dev), after=after)
    lifespans = dict(lifespans=torch.as_tensor(rng.randint(0, 5, (N, A)).astype(np.int32), device=dev),
                     max_lifespans=torch.full((N, A), 4, dtype=torch.int32, device=dev),
                     fresh=torch.as_tensor(rng.randint(5, 9, (N, A)).astype(np.int32), device=dev))
    imu = (torch.zeros((N, A, 3), device=dev), 360., 10.)
    table = torch.tensor(TABLE, dtype=torch.float32, device=dev)
    actions = torch.as_tensor(rng.randint(0, 5, (N, A)), device=dev)
    p = both(c, movement=(actions, table, .875), respawn=respawn, lifespans=lifespans, imu=imu)
    assert respawn['mask'].any() and not respawn['mask'].all() and (p.progress < 1).any()
    # ... and the respawn alone, without lifespans or movement
    respawn['mask'] = torch.as_tensor(rng.rand(N, A) < .3, device=dev)
    util.random_velocities(c, rng, speed=3., spin=0.)
    both(c, respawn=respawn, imu=imu)


def test_step_render_is_the_slide_launch_then_render():
    from megastep_amd import _lib, cuda
    from tests.test_gpu_step_render import _world as render_world
    for n_agents, res in ((1, 64), (3, 128)):                            # (1, 64): the shape the plain step takes as one launch
        c, _ = render_world(16, n_agents, res, 130., seed=12)
        util.random_velocities(c, np.random.RandomState(13), speed=4.)
        start = _state(c)
        lines = c.scenery.lines.vals.clone()
        p1 = cuda.physics(c.scenery, c.agents, slide=True)
        r1 = cuda.render(c.scenery, c.agents)
        two = _state(c) + [c.scenery.lines.vals.clone()]
        _restore(c, start)
        c.scenery.lines.vals.copy_(lines)
        cuda.step_render(c.scenery, c.agents)                            # (sets the one-launch flag where the shape allows)
        _restore(c, start)
        c.scenery.lines.vals.copy_(lines)
        p2, r2 = cuda.step_render(c.scenery, c.agents, slide=True)
        assert _lib.lib().ms_debug_last_step_fused() == 0
        for x, y in zip(_state(c) + [c.scenery.lines.vals], two):
            util.assert_bits(x, y)
        for k in ('progress', 'slid', 'stopped'):
            util.assert_bits(getattr(p2, k), getattr(p1, k), k)
        for k in cuda.FIELDS:
            util.assert_bits(getattr(r2, k), getattr(r1, k), k)
        assert (p1.slid > 0).any()


def test_call_plumbing():
    from megastep_amd import cuda
    c, _ = _world(6, 2, seed=14)
    rng = np.random.RandomState(15)
    util.random_velocities(c, rng, speed=3.)
    start = _state(c)
    first = cuda.physics(c.scenery, c.agents, slide=True)
    assert first.slid.dtype == torch.float32 and first.stopped.dtype == torch.uint8 and first.slid.shape == first.stopped.shape == (6, 2)
    after = _state(c)
    held = [t.clone() for t in (first.progress, first.slid, first.stopped)]
    assert cuda.physics(c.scenery, c.agents).slid is None                # (a plain step has neither)
    # out=: rewritten in place
    ptrs = [t.data_ptr() for t in (first.progress, first.slid, first.stopped)]
    _restore(c, start)
    c.agents.velocity[:] = -c.agents.velocity
    again = cuda.physics(c.scenery, c.agents, slide=dict(bounce=.05), out=first)
    assert again is first and ptrs == [t.data_ptr() for t in (first.progress, first.slid, first.stopped)]
    assert not util.same_bits(first.progress, held[0]).all()
    with pytest.raises(RuntimeError, match='out'):
        cuda.physics(c.scenery, c.agents, slide=True, out=cuda.physics(c.scenery, c.agents))
    # a side stream
    _restore(c, start)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        aside = cuda.physics(c.scenery, c.agents, slide=True)
    side.synchronize()
    for x, y in zip(_state(c) + [aside.progress, aside.slid, aside.stopped], after + held):
        util.assert_bits(x, y)
    # a captured graph, replayed three times: each replay steps the agents on from where the last left them
    _restore(c, start)
    static = cuda.physics(c.scenery, c.agents, slide=True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cuda.physics(c.scenery, c.agents, slide=True, out=static)
    _restore(c, start)
    replayed = []
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        replayed.append(_state(c) + [static.progress.clone(), static.slid.clone(), static.stopped.clone()])
    _restore(c, start)
    for k in range(3):
        eager = cuda.physics(c.scenery, c.agents, slide=True)
        for x, y in zip(replayed[k], _state(c) + [eager.progress, eager.slid, eager.stopped]):
            util.assert_bits(x, y, f'replay {k}')


class _Follower:
    """An env whose step is the path follower's: the decision handed in is ignored."""

    def __init__(self, env):
        self.env = env

    def __getattr__(self, name):
        return getattr(self.env, name)

    def step(self, decision):
        return self.env.step(self.env.expert())


def test_pointgoal_slides_eagerly_and_as_a_graph():
    from megastep_amd import arrdict, graphs
    from megastep_amd.demo import PointGoal
    from tests.test_navfield_host import plans
    logs, slid = [], 0
    for graphed in (False, True):
        torch.manual_seed(3); np.random.seed(3)
        env = PointGoal(64, geometries=plans(64), max_lifespan=10**6, slide=True)
        assert env._mover.slide is True
        stepper = graphs.GraphedStep(_Follower(env), warmup=3) if graphed else _Follower(env)
        stepper.reset()
        env.expert()                                                     # (the expert and its buffers are made outside the graph)
        nothing = arrdict.arrdict(actions=torch.zeros((64, 1), dtype=torch.long, device='cuda'))
        log = []
        for _ in range(20 if graphed else 23):
            world = stepper.step(nothing)
            log.append([world.reward.clone(), world.reset.clone(), world.obs.goal.clone(), env.core.agents.positions.clone(),
                        env.core.agents.angles.clone(), env.core.agents.velocity.clone()])
        logs.append(log)
    eager, graphed = logs
    # the graphed env's first step call is four steps (three of warm-up and the captured one): its k-th is the eager env's k + 3
    for k in range(len(graphed)):
        for x, y in zip(graphed[k], eager[k + 3]):
            util.assert_bits(x, y, f'step {k}')
    assert not torch.equal(eager[0][3], eager[-1][3])


def test_defaults_build_what_they_built():
    from megastep_amd.demo import PointGoal
    from tests.test_navfield_host import plans
    env = PointGoal(4, geometries=plans(4))
    assert env._mover.slide is None


def test_arguments_are_refused():
    from megastep_amd import _lib, cuda
    c, _ = _world(2, 1, seed=16)
    for slide in (dict(bounce=-.1), dict(bounce=1.5), dict(bounce=float('nan')), dict(bouncy=1), 'yes'):
        with pytest.raises(RuntimeError):
            cuda.physics(c.scenery, c.agents, slide=slide)
    # ... and by the library itself, before anything is launched
    h = _lib.lib()
    before = _state(c)
    progress = torch.zeros((2, 1), device='cuda')
    args = (C.byref(c.scenery._as_struct()), C.byref(c.agents._plain), None, None)
    for bounce in (-.1, 1.5, float('nan')):
        assert h.ms_slide_physics(*args, C.byref(_lib.MsSlide(bounce, None, None)), progress.data_ptr(), C.byref(c.config), None) == -1
    assert h.ms_slide_physics(*args, None, progress.data_ptr(), C.byref(c.config), None) == -1
    crowd, _ = util.plan_world(1, 65, 64, 130., seed=3, toy='box')
    with pytest.raises(RuntimeError, match='not supported'):
        cuda.physics(crowd.scenery, crowd.agents, slide=True)
    torch.cuda.synchronize()
    for x, y in zip(_state(c), before):
        util.assert_bits(x, y)


ROLLED = ('positions', 'angles', 'velocity', 'angvelocity', 'progress', 'stops', 'first_stop', 'trail', 'slides')


def _stepped(c, actions, table, keep):
    """The reference of a sliding rollout with the others at rest: for every agent a and candidate k the agents restored, everyone
    but a at zero velocity and the no-op action, then H sliding calls of cuda.physics. Returns the nine outputs as tensors."""
    from megastep_amd import cuda
    N, A = c.agents.angles.shape
    K, H = actions.shape[-2:]
    start = _state(c)
    dev = 'cuda'
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)
    out = dict(positions=torch.empty((N, A, K, 2), device=dev), angles=torch.empty((N, A, K), device=dev), velocity=torch.empty((N, A, K, 2), device=dev),
               angvelocity=torch.empty((N, A, K), device=dev), progress=torch.empty((N, A, K), device=dev), stops=i32(N, A, K),
               first_stop=i32(N, A, K), trail=torch.empty((N, A, K, H, 2), device=dev), slides=i32(N, A, K))
    for a in range(A):
        only = torch.zeros((N, A), dtype=torch.bool, device=dev)
        only[:, a] = True
        for k in range(K):
            _restore(c, start)
            c.agents.velocity[:] = torch.where(only[..., None], start[2], torch.zeros_like(start[2]))
            c.agents.angvelocity[:] = torch.where(only, start[3], torch.zeros_like(start[3]))
            least = torch.ones(N, device=dev)
            stops, slides, first = i32(N), i32(N), torch.full((N,), H, dtype=torch.int32, device=dev)
            for h in range(H):
                act = torch.where(only, actions[:, :, k, h], torch.zeros_like(actions[:, :, k, h])).contiguous()
                rest = c.agents.positions.clone()
                p = cuda.physics(c.scenery, c.agents, movement=(act, table, keep), slide=True)
                # (the others stand still for the whole horizon: a runs into them, they do not give way)
                c.agents.positions[:] = torch.where(only[..., None], c.agents.positions, rest)
                c.agents.velocity[:] = torch.where(only[..., None], c.agents.velocity, torch.zeros_like(rest))
                c.agents.angvelocity[:] = torch.where(only, c.agents.angvelocity, torch.zeros_like(c.agents.angvelocity))
                c.agents.angles[:] = torch.where(only, c.agents.angles, start[1])
                least = torch.minimum(least, p.progress[:, a])
                dead = p.stopped[:, a] > 0
                stops += dead.int()
                slides += (~dead & (p.slid[:, a] > 0)).int()
                first = torch.where(dead & (first == H), torch.full_like(first, h), first)
                out['trail'][:, a, k, h] = c.agents.positions[:, a]
            out['positions'][:, a, k], out['angles'][:, a, k] = c.agents.positions[:, a], c.agents.angles[:, a]
            out['velocity'][:, a, k], out['angvelocity'][:, a, k] = c.agents.velocity[:, a], c.agents.angvelocity[:, a]
            out['progress'][:, a, k], out['stops'][:, a, k], out['first_stop'][:, a, k], out['slides'][:, a, k] = least, stops, first, slides
    _restore(c, start)
    return out


def test_rollouts_that_slide_are_slide_calls_on_restored_agents():
    """cuda.rollouts(slide=) against K H sliding steps, at candidate counts round a wave's 64 lanes and at the count where the
    plain call would change its scheme; with and without a wall grid; and the mover's own rollouts."""
    from megastep_amd import cuda
    N, A, H = 5, 2, 3
    c, _ = _world(N, A, seed=9)
    _odd_poses(c, np.random.RandomState(10))
    c.agents.positions[0, 1] = c.agents.positions[0, 0] + torch.tensor([.25, .05], device='cuda')
    g = torch.Generator().manual_seed(4)
    actions = torch.randint(0, 7, (N, A, 65, H), generator=g).cuda()
    table = torch.tensor(TABLE, dtype=torch.float32, device='cuda')
    before = _state(c)
    whole = cuda.rollouts(c.scenery, c.agents, actions, table, keep=.875, others='rest', trail=True, slide=True)
    for x, y in zip(_state(c), before):
        util.assert_bits(x, y, 'the agents after a call')
    want = _stepped(c, actions, table, .875)
    for k in ROLLED:
        util.assert_bits(getattr(whole, k), want[k], k)
    assert (whole.slides > 0).any() and (whole.stops > 0).any() and (whole.stops == 0).any()
    for K in (1, 25, 64):
        part = cuda.rollouts(c.scenery, c.agents, actions[:, :, :K].contiguous(), table, keep=.875, others='rest', trail=True, slide=dict(bounce=.05))
        for k in ROLLED:
            util.assert_bits(getattr(part, k), getattr(whole, k)[:, :, :K].contiguous(), f'K = {K}: {k}')
    plain = cuda.rollouts(c.scenery, c.agents, actions, table, keep=.875, others='rest', trail=True)
    assert plain.slides is None and not util.same_bits(plain.positions, whole.positions).all()
    with pytest.raises(RuntimeError, match='out'):
        cuda.rollouts(c.scenery, c.agents, actions, table, keep=.875, others='rest', trail=True, slide=True, out=plain)
    # without a wall grid: the same bits
    bare, _ = _world(N, A, seed=9, grid=False)
    _restore(bare, before)
    swept = cuda.rollouts(bare.scenery, bare.agents, actions, table, keep=.875, others='rest', trail=True, slide=True)
    for k in ROLLED:
        util.assert_bits(getattr(swept, k), getattr(whole, k), f'no grid: {k}')


def test_the_other_scheme_is_refused_with_slide():
    from megastep_amd import _lib, cuda
    c, _ = _world(2, 1, seed=16)
    actions = torch.zeros((3, 2), dtype=torch.int64, device='cuda')
    table = torch.tensor(TABLE, dtype=torch.float32, device='cuda')
    h = _lib.lib()
    try:
        assert h.ms_debug_rollout_scheme(1) == 0
        with pytest.raises(RuntimeError, match='invalid argument'):
            cuda.rollouts(c.scenery, c.agents, actions, table, slide=True)
        cuda.rollouts(c.scenery, c.agents, actions, table)
        assert h.ms_debug_rollout_scheme(0) == 0
        cuda.rollouts(c.scenery, c.agents, actions, table, slide=True)
    finally:
        h.ms_debug_rollout_scheme(-1)
    for slide in (dict(bounce=2.), 'yes'):
        with pytest.raises(RuntimeError):
            cuda.rollouts(c.scenery, c.agents, actions, table, slide=slide)
