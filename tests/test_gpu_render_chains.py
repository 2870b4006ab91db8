"""The render kernel's serial chains ("a window's LDS reads"): pass 2 asks for a window's list entries a window
ahead and for `near` together with `ray`, and the colour leaves as one 12-byte store a lane.  None of it may move a bit: every requested plane and the agents' drawn lines against the oracle, at the smallest
shapes where each can go wrong - pair counts on and next to a window's edge, a list worked off twice, a ray group without
pairs, a last group of fewer than 64 rays, a `screen` that ends where its allocation ends, and 1, 4 and 64 agents an env with
models of 1 and 4 lines."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import util

pytestmark = pytest.mark.gpu

PLANES = ('indices', 'locations', 'dots', 'distances', 'screen')


@pytest.fixture
def groups():
    from megastep_amd import _lib
    h = _lib.lib()

    def pin(g, tail_envs=0):
        h.ms_debug_ray_groups(g)
        h.ms_debug_ray_group_tail(-1., tail_envs)
    yield pin
    h.ms_debug_ray_groups(0)
    h.ms_debug_ray_group_tail(-1., -1)


def _oracle(c):
    """The oracle's frame of the world as it stands, and the lines it leaves behind (the agents' rows drawn)."""
    ref = util.OracleWorld(c)
    ref.pull_baked(c)
    want = ref.render()
    return want, ref.scene.lines_vals.copy()


def _holds(c, frame, want, lines, planes=PLANES, what=''):
    for k in planes:
        if k == 'indices':
            np.testing.assert_array_equal(util._np(frame.indices), want[k], err_msg=f'{what} hit indices differ')
        else:
            util.assert_bits(getattr(frame, k), want[k], f'{what} {k}')
    util.assert_bits(c.scenery.lines.vals, lines, f'{what} lines')


def _hand_made_world(walls_per_env, n_agents, res, fov, positions, angles, grid=True):
    """util.custom_world - hand-made wall sets, agents placed explicitly - baked with or without the wall grid (without: every
    wave meets every wall, whatever hides it)."""
    from megastep_amd import arrdict, core, cuda, scene
    geoms = [arrdict.arrdict(walls=np.asarray(w, float), lights=np.array([[2., 2.]]), masks=np.ones((4, 4), np.int16), res=.2)
             for w in walls_per_env]
    np.random.seed(0)
    scenery = scene.scenery(geoms, n_agents, device='cuda', random=np.random.RandomState(0), bake=False)
    cuda.bake(scenery, wall_grid=grid)
    assert (scenery._wg is not None) == grid
    c = core.Core(scenery, res=res, fov=fov, fps=10)
    c.agents.positions[:] = torch.as_tensor(np.asarray(positions, np.float32), device=c.device)
    c.agents.angles[:] = torch.as_tensor(np.asarray(angles, np.float32), device=c.device)
    return c


# ---- steps 1 and 2: pass 2's windows --------------------------------------------------------------------------------------

def test_a_single_full_window_on_a_floorplan():
    from megastep_amd import cuda
    c, _ = util.plan_world(2, 2, 64, 130, seed=5)
    want, lines = _oracle(c)
    _holds(c, cuda.render(c.scenery, c.agents), want, lines)


def _pairs_on_the_host(walls, pose_xy, angle, res, fov, radius):
    """The (line, ray) pairs pass 1 gives a lone agent's 64-ray wave among `walls` (W, 4): the sum of ray_interval's counts."""
    from megastep_amd import _lib
    lib = _lib.lib()
    f32p = C.POINTER(C.c_float)
    s_, c_ = C.c_float(), C.c_float()
    lib.ms_host_sincospi(float(np.float32(angle)/np.float32(180.)), C.byref(s_), C.byref(c_))
    pose = np.array([pose_xy[0], pose_xy[1], s_.value, c_.value], np.float32)
    total = 0
    for w in np.asarray(walls, np.float32).reshape(-1, 4):
        lo, n = C.c_int(), C.c_int()
        lib.ms_host_ray_interval(pose.ctypes.data_as(f32p), w.ctypes.data_as(f32p), res, fov, radius, 0, C.byref(lo), C.byref(n))
        total += n.value
    return total


def _rooms(layers, closed):
    """`layers` square rooms round (2.5, 2.5), 3 m and 3.6 m wide; open ones lack their east wall."""
    walls = []
    for half in (1.5, 1.8)[:layers]:
        lo, hi = 2.5 - half, 2.5 + half
        room = [[[lo, lo], [hi, lo]], [[hi, hi], [lo, hi]], [[lo, hi], [lo, lo]]]
        if closed:
            room.append([[hi, lo], [hi, hi]])
        walls += room
    return np.array(walls, float)


def _heading_with(walls, xy, target, res, fov, radius):
    """A heading at which the wave has `target` pairs - the middle one of three neighbours a twentieth of a degree apart that all
    have (the device's cull takes its reciprocals from the hardware, the host's divides: no heading where a last bit decides)."""
    angles = np.arange(-180., 180., .05)
    on = np.array([_pairs_on_the_host(walls.reshape(-1, 4), xy, a, res, fov, radius) == target for a in angles])
    run = on[:-2] & on[1:-1] & on[2:]
    assert run.any(), f'no heading gives {target} pairs'
    return float(angles[np.argmax(run) + 1])


@pytest.mark.parametrize('layers', [1, 2])
@pytest.mark.parametrize('off', [0, -1, 1])
def test_pair_counts_on_and_next_to_a_windows_edge(layers, off):
    """A lone agent in a square room: every ray meets one wall's interval, 64 pairs - one full window, behind which the window
    ahead is an entry read and thrown away; a corner on a ray makes 65, a missing wall with one ray through the gap 63.  Two rooms,
    one inside the other, without the wall grid (whose lists would drop the outer one): 128, 129 and 127 pairs - the second
    window's entries follow from the marks of the first (`before`)."""
    from megastep_amd import core, cuda
    xy, res, fov = (2.3, 2.7), 64, 130.
    walls = _rooms(layers, closed=off >= 0)
    target = 64*layers + off
    angle = _heading_with(walls, xy, target, res, fov, core.AGENT_RADIUS)
    c = _hand_made_world([walls], 1, res, fov, [[xy]], [[angle]], grid=layers == 1)
    want, lines = _oracle(c)
    frame = cuda.render(c.scenery, c.agents, telemetry=True)
    pairs, windows = frame._telemetry[3:5].tolist()
    assert (pairs, windows) == (target, (target + 63)//64)
    _holds(c, frame, want, lines)
    _holds(c, cuda.render(c.scenery, c.agents), want, lines, what='without a workspace')


def test_a_list_that_is_worked_off_twice():
    """150 walls in three staggered arcs in front of a lone agent, each wide enough to hold a ray's direction, and no wall grid:
    more lines with pairs than the wave's list holds (MS_VCAP = 128), so pass 2 runs when the list is full and again at the end."""
    from megastep_amd import cuda
    res, fov, p = 64, 130., np.array([5., 5.])
    theta = np.radians(np.linspace(-55, 55, 150))
    rho = 2. + .5*(np.arange(150) % 3)
    mid = p + rho[:, None]*np.stack([np.cos(theta), np.sin(theta)], -1)
    half = (rho*np.tan(np.radians(2.5)))[:, None]*np.stack([-np.sin(theta), np.cos(theta)], -1)
    walls = np.stack([mid - half, mid + half], 1)
    # each wall's directions hold a ray's (the rays: atan of 64 evenly spaced screen points), so each has pairs with the wave
    rays = np.arctan((res - 2*np.arange(res) - 1)*np.tan(np.radians(fov/2))/res)
    holds_a_ray = ((rays[None] > theta[:, None] - np.radians(2.4)) & (rays[None] < theta[:, None] + np.radians(2.4))).any(1)
    assert holds_a_ray.sum() >= 140
    c = _hand_made_world([walls], 1, res, fov, [[p]], [[0.]], grid=False)
    want, lines = _oracle(c)
    frame = cuda.render(c.scenery, c.agents, telemetry=True)
    pairs, windows = frame._telemetry[3:5].tolist()
    assert pairs >= 140 and windows >= 2, (pairs, windows)
    _holds(c, frame, want, lines)
    assert len(np.unique(util._np(frame.indices))) > 40, 'a view of many walls'


def test_a_ray_group_without_pairs_in_a_wave_of_four(groups):
    """256 rays as one wave of four groups: in the second env a single wall in the second group's rays - the other three groups have
    no pairs at all, and their pass 2 is a loop that never runs."""
    from megastep_amd import _lib, cuda
    room = _rooms(1, closed=True)
    lone = np.array([[[4., 3.2], [4., 4.5]]])
    c = _hand_made_world([room, lone], 1, 256, 130., [[[2.3, 2.7]], [[2., 2.5]]], [[20.], [0.]])
    want, lines = _oracle(c)
    idx = want['indices'][1, 0]
    assert (idx[64:128] >= 0).any() and (idx[:64] < 0).all() and (idx[128:] < 0).all()
    groups(4)
    frame = cuda.render(c.scenery, c.agents)
    assert _lib.lib().ms_debug_last_render_groups() == 4
    _holds(c, frame, want, lines)
    groups(1)
    _holds(c, cuda.render(c.scenery, c.agents), want, lines, what='one group a wave')


# ---- step 3: the colour store --------------------------------------------------------------------------------------------

@pytest.mark.parametrize('res,pinned', [(40, 0), (100, 1), (100, 0), (100, 4)])
def test_a_last_group_of_fewer_than_64_rays(groups, res, pinned):
    from megastep_amd import cuda
    c, _ = util.plan_world(3, 3, res, 90, seed=9)
    want, lines = _oracle(c)
    groups(pinned)
    _holds(c, cuda.render(c.scenery, c.agents), want, lines)
    only = cuda.render(c.scenery, c.agents, fields=('screen',))
    util.assert_bits(only.screen, want['screen'], 'screen alone')


@pytest.mark.parametrize('fields', [None, ('screen',)])
@pytest.mark.parametrize('res', [64, 100])
def test_the_colour_store_ends_where_screen_ends(fields, res):
    """`screen` as the first N A R 3 floats of a buffer with 1024 canary floats behind them: the last lane's 12 bytes are the
    buffer's last, and nothing lands behind them - with every plane wanted and with `screen` alone (the instantiation of
    optional outputs)."""
    from megastep_amd import cuda
    c, _ = util.plan_world(2, 2, res, 130, seed=3, toy='box')
    want, lines = _oracle(c)
    N, A = c.n_envs, c.n_agents
    size, canary = N*A*res*3, 1024
    buf = torch.full((size + canary,), -7., device=c.device)
    frame = cuda.render(c.scenery, c.agents, fields=fields)
    frame._struct.screen = buf.data_ptr()
    frame = cuda.render(c.scenery, c.agents, fields=fields, out=frame)
    torch.cuda.synchronize()
    assert bool((buf[size:] == -7.).all()), 'the render wrote behind the end of screen'
    got = buf[:size].view(N, A, res, 3)
    assert (want['indices'][-1, -1, -1] >= 0) and (want['screen'][-1, -1, -1] > 0).any(), 'the last ray shows a wall'
    util.assert_bits(got[-1, -1, -1], want['screen'][-1, -1, -1], 'the last ray')
    util.assert_bits(got, want['screen'], 'screen')
    _holds(c, frame, want, lines, planes=[k for k in (fields or PLANES) if k != 'screen'])


# ---- the draw step --------------------------------------------------------------------------------------------------------

def _modelled_world(model, n_agents, room, seed):
    """A box of `room` metres with `n_agents` agents whose outline is `model` (M, 2, 2) instead of the product's eight lines."""
    from megastep_amd import core, cuda, scene
    rng = np.random.RandomState(seed)
    model = np.asarray(model, np.float32)
    lo, hi = 1., 1. + room
    walls = np.array([[[lo, lo], [hi, lo]], [[hi, lo], [hi, hi]], [[hi, hi], [lo, hi]], [[lo, hi], [lo, lo]]], np.float32)
    lines = np.concatenate([np.tile(model, (n_agents, 1, 1)), walls])
    widths = scene.resolutions(lines.astype(float)).astype(np.int32)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device='cuda')
    scenery = cuda.Scenery(
        n_agents=n_agents,
        lights=cuda.Ragged2D(t(np.array([[lo + room/2, lo + room/2, 1.2], [lo + 1, hi - 1, .8]], np.float32)), t(np.array([2], np.int32))),
        lines=cuda.Ragged3D(t(lines), t(np.array([len(lines)], np.int32))),
        textures=cuda.Ragged2D(t(rng.uniform(.05, 1., (int(widths.sum()), 3)).astype(np.float32)), t(widths)),
        model=t(model))
    cuda.bake(scenery)
    c = core.Core(scenery, res=64, fov=130, fps=10)
    c.agents.positions[:] = t(rng.uniform(lo + .5, hi - .5, (1, n_agents, 2)).astype(np.float32))
    c.agents.angles[:] = t(rng.uniform(-180, 180, (1, n_agents)).astype(np.float32))
    return c


@pytest.mark.parametrize('n_model', [1, 4])
@pytest.mark.parametrize('n_agents', [1, 4, 64])
def test_the_draw_step_with_models_of_one_and_four_lines(n_agents, n_model):
    """The rows a render publishes - the draw step (agent_line_m; doing it from the wave's own scalars was measured and not kept,
    DESIGN 3.6) - for 1, 4 and 64 agents an env, whose outline has 1 or 4 lines."""
    from megastep_amd import cuda
    from megastep_amd import scene
    model = scene.agent_model()[::8//n_model][:n_model]
    c = _modelled_world(model, n_agents, 4. if n_agents < 64 else 12., seed=n_agents + n_model)
    AF = n_agents*n_model
    c.scenery.lines.vals[:AF] = 0.                                           # (what the render must draw over)
    want, lines = _oracle(c)
    frame = cuda.render(c.scenery, c.agents)
    util.assert_bits(c.scenery.lines.vals[:AF], lines[:AF], 'the agents\' rows')
    _holds(c, frame, want, lines)
