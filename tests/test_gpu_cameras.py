"""Cameras on the GPU (`cuda.shade`, `cuda.cameras`, `cuda.mounted`, `cuda.look`, `modules.Cameras`, `PointGoal(panorama=True)`):
plane cameras mounted at the agents' own poses give the render, every plane bit for bit, with the light grid and without;
`shade_kernel` gives `ms_host_shade`'s bits on rays the render cannot cast - fixed cameras watching single-agent sceneries, rings
of 360 degrees, ray counts that straddle waves and envs, 65 lights; the rays of free cameras are what they are said to be; and
everything reuses its buffers, runs on a side stream and replays in a HIP graph."""
import numpy as np
import pytest
import torch

from tests import shade_rule as S
from tests import util

pytestmark = pytest.mark.gpu

F = np.float32
PLANES = ('indices', 'locations', 'dots', 'distances')


def _bits(t):
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().numpy()
    return np.ascontiguousarray(t).view(np.int32)


def _agent_rows(c):
    return c.scenery.n_agents*c.scenery.model.shape[0]


# ---- the condition the feature rests on: look from the agents' own poses is the render ------------------------------------------
@pytest.mark.parametrize('light_grid', [True, False])
@pytest.mark.parametrize('n_envs,res,seed', S.LOOK_WORLDS)
def test_plane_cameras_at_the_agents_poses_see_the_render(n_envs, res, seed, light_grid):
    from megastep_amd import cuda
    c = S.triangle_world(n_envs, res, seed, 'cuda')
    assert c.scenery._as_struct().lg_vals                                   # (a scenery of three agents carries a light grid)
    r = cuda.render(c.scenery, c.agents)
    before = c.scenery.lines.vals.clone()
    cams = cuda.mounted(c.agents, [[0., 0., 0.]], c.res, c.fov)
    seen = cuda.look(c.scenery, cams, agents=c.agents, fields=('screen',) + PLANES, light_grid=light_grid)
    assert torch.equal(c.scenery.lines.vals.view(torch.int32), before.view(torch.int32))
    for k in PLANES + ('screen',):
        assert getattr(seen, k).shape == getattr(r, k).shape, k
        assert np.array_equal(_bits(getattr(seen, k)), _bits(getattr(r, k))), k
    on_body = (r.indices >= 0) & (r.indices < _agent_rows(c))
    assert int(on_body.sum()) > 20 and bool((r.screen[on_body] > 0).any())
    assert seen.agents is None and cams.n_cameras == 3


# ---- shade_kernel against the host statement on rays the render cannot cast ------------------------------------------------------------
def _assert_kernel_is_host(c, cams, light_grid=True, rule_envs=()):
    """look through `cams`: the screen is ms_host_shade's on the planes the raycast wrote - with the agents, and without - and,
    in `rule_envs`, the numpy rule's.  Returns the Look."""
    from megastep_amd import cuda
    before = c.scenery.lines.vals.clone()
    seen = cuda.look(c.scenery, cams, agents=c.agents, fields=('screen', 'indices', 'locations', 'dots'), light_grid=light_grid)
    assert torch.equal(c.scenery.lines.vals.view(torch.int32), before.view(torch.int32))
    scene, agents = util.scene_dict(c.scenery), util.agents_dict(c.agents)
    n = len(c.scenery.lines)
    planes = [getattr(seen, k).reshape(n, -1).cpu().numpy() for k in ('indices', 'locations', 'dots')]
    got = seen.screen.reshape(n, -1, 3)
    assert np.array_equal(_bits(got), _bits(S.host_shade(scene, agents, *planes)))
    hits = cuda.Raycast(*(getattr(seen, k).reshape(n, -1) for k in ('indices', 'locations', 'dots')), None, None)
    bare = cuda.shade(c.scenery, hits, light_grid=light_grid)
    assert np.array_equal(_bits(bare), _bits(S.host_shade(scene, None, *planes)))
    if rule_envs:
        want = S.shade_rule(scene, S.draw_rows(scene, agents), *planes)
        for e in rule_envs:
            assert np.array_equal(_bits(got[e]), _bits(want[e])), e
    return seen


def _watchers(c, offsets, headings):
    """Fixed camera poses (N, C, 3): camera k of every env stands at the first agent's position + offsets[k], heading headings[k]."""
    p = c.agents.positions[:, :1, :] + torch.as_tensor(offsets, dtype=torch.float32, device='cuda')[None]
    h = torch.as_tensor(headings, dtype=torch.float32, device='cuda')[None, :, None].expand(p.shape[0], -1, 1)
    return torch.cat([p, h], -1).contiguous()


@pytest.mark.parametrize('toy', ['box', None])
def test_fixed_cameras_watch_the_agent_of_single_agent_sceneries(toy):
    """One agent per env: such a scenery has no light grid, its render never lights a body - a camera beside the agent does."""
    from megastep_amd import cuda
    c, _ = util.plan_world(4, 1, 64, 130, seed=41, toy=toy)
    assert not c.scenery._as_struct().lg_vals
    poses = _watchers(c, [[.7, 0.], [0., -.5]], [180., 90.])
    for res, fov, projection in ((64, 70., 'plane'), (37, 120., 'ring')):
        seen = _assert_kernel_is_host(c, cuda.cameras(poses, res, fov, projection), rule_envs=(0,))
        on_body = (seen.indices >= 0) & (seen.indices < _agent_rows(c))
        assert int(on_body.sum()) > 8 and bool((seen.screen[on_body] > 0).any())


@pytest.mark.parametrize('light_grid', [True, False])
@pytest.mark.parametrize('R', [1, 37, 64, 65, 200])
def test_rings_of_every_size_with_and_without_the_grid(R, light_grid):
    """A panorama on every agent of a three-agent world: 3 R rays an env, so waves straddle envs unless 3 R is a multiple of 64."""
    from megastep_amd import cuda
    c = S.triangle_world(5, 64, 33, 'cuda')
    cams = cuda.mounted(c.agents, [[0., 0., 10.]], R, 360., 'ring')
    seen = _assert_kernel_is_host(c, cams, light_grid=light_grid, rule_envs=(4,) if R == 37 else ())
    if R >= 37:
        assert int(((seen.indices >= 0) & (seen.indices < _agent_rows(c))).sum()) > 0


def test_one_env_and_sixty_five_lights():
    from megastep_amd import cuda
    rng = np.random.RandomState(5)
    c = util.many_lights_world(util.many_lights_geometries(rng), rng)          # 70, 9, 150 and 64 lights
    poses = _watchers(c, [[1.2, .4], [-.3, 1.5]], [200., -80.])
    for light_grid in (True, False):
        seen = _assert_kernel_is_host(c, cuda.cameras(poses, 100, 360., 'ring'), light_grid=light_grid, rule_envs=(1,))
        assert int(((seen.indices >= 0) & (seen.indices < _agent_rows(c))).sum()) > 8
    one = S.triangle_world(1, 64, 34, 'cuda')
    for light_grid in (True, False):
        seen = _assert_kernel_is_host(one, cuda.mounted(one.agents, [[0., 0., 0.], [-.05, 0., 180.]], 65, 150., 'ring'), light_grid=light_grid)
        assert int(((seen.indices >= 0) & (seen.indices < _agent_rows(one))).sum()) > 0


# ---- the rays of free cameras -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('res,fov', [(64, 130.), (37, 70.)])
def test_plane_cameras_at_the_agents_poses_cast_the_renders_rays(res, fov):
    from megastep_amd import core, cuda
    c, _ = util.plan_world(6, 3, res, fov, seed=3)
    n, a = c.agents.angles.shape
    poses = torch.cat([c.agents.positions, c.agents.angles[..., None]], -1).contiguous()
    cams = cuda.cameras(poses, res, fov)
    assert cams.poses is poses and cams.origins.shape == cams.directions.shape == (n, a*res, 2)
    assert np.array_equal(_bits(cams.directions.view(n, a, res, 2)), _bits(cuda.camera_rays(c.agents)))
    assert np.array_equal(_bits(cams.origins.view(n, a, res, 2)), _bits(c.agents.positions[:, :, None, :].expand(n, a, res, 2)))
    mounted = cuda.mounted(c.agents, [[0., 0., 0.]], res, fov)
    assert np.array_equal(_bits(mounted.poses), _bits(poses))                # a mount of zeros leaves the agent's pose exactly
    assert np.array_equal(_bits(mounted.directions), _bits(cams.directions))
    # update() follows the poses, in place
    at = cams.directions.data_ptr()
    util.random_velocities(c, np.random.RandomState(0))
    cuda.physics(c.scenery, c.agents)
    poses.copy_(torch.cat([c.agents.positions, c.agents.angles[..., None]], -1))
    assert cams.update() is cams and cams.directions.data_ptr() == at
    assert np.array_equal(_bits(cams.directions.view(n, a, res, 2)), _bits(cuda.camera_rays(c.agents)))
    assert np.array_equal(_bits(mounted.update().directions), _bits(cams.directions))


def _ring64(headings, res, fov):
    """The ring's unit vectors restated in binary64 from the binary32 headings: (..., res, 2)."""
    r = np.arange(res, dtype=np.float64)
    deg = np.asarray(headings, np.float64)[..., None] + fov*(res - 2*r - 1)/(2*res)
    return np.stack([np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))], -1)


#: the worst deviation of a ring direction's component from the binary64 restatement, as measured on an MI355X over the test's
#: 37-ray, 210-degree rings at 4096 random headings, and the margin the test holds: four times that
RING_WORST = 6.504e-7
RING_MARGIN = 4*RING_WORST


def test_the_ring_is_exact_at_quarter_turns_and_near_binary64_elsewhere():
    from megastep_amd import cuda
    poses = torch.tensor([[[1., 2., 0.], [3., 4., 90.], [5., 6., 180.], [7., 8., 270.]]], device='cuda')
    cams = cuda.cameras(poses, 2, 360., 'ring')
    d = cams.directions.view(4, 2, 2).cpu().numpy()
    left = np.array([[0, 1], [-1, 0], [0, -1], [1, 0]], F)                    # ray 0: a quarter turn to the left of the heading
    assert np.array_equal(d[:, 0], left) and np.array_equal(d[:, 1], -left)
    assert np.array_equal(cams.origins.view(4, 2, 2).cpu().numpy(), poses[0, :, None, :2].expand(4, 2, 2).cpu().numpy())
    rng = np.random.RandomState(9)
    headings = rng.uniform(-360, 360, (64, 64)).astype(F)
    poses = torch.as_tensor(np.concatenate([rng.uniform(0, 9, (64, 64, 2)).astype(F), headings[..., None]], -1), device='cuda')
    got = cuda.cameras(poses, 37, 210., 'ring').directions.view(64, 64, 37, 2).cpu().numpy()
    worst = float(np.abs(got.astype(np.float64) - _ring64(headings, 37, 210.)).max())
    print(f'ring: worst deviation from binary64 {worst:.3e}, margin {RING_MARGIN:.3e}')
    assert worst <= RING_MARGIN
    assert float(np.abs(np.sqrt((got.astype(np.float64)**2).sum(-1)) - 1).max()) <= RING_MARGIN      # unit vectors
    a, b = got[:, :, :-1].astype(np.float64), got[:, :, 1:].astype(np.float64)
    assert (a[..., 0]*b[..., 1] - a[..., 1]*b[..., 0] < 0).all()                 # ray 0 leftmost: each next ray turns clockwise


# ---- buffers, streams, graphs ------------------------------------------------------------------------------------------------------------
def test_look_reuses_its_buffers_runs_on_a_side_stream_and_replays_in_a_graph():
    from megastep_amd import cuda
    c = S.triangle_world(5, 64, 35, 'cuda')
    fields = ('screen', 'distances', 'agents')
    cams = cuda.mounted(c.agents, [[0., 0., 0.], [-.02, 0., 180.]], 48, 100.)
    out = cuda.look(c.scenery, cams, agents=c.agents, fields=fields)
    assert out.screen.shape == (5, 6, 48, 3) and out.distances.shape == out.agents.shape == (5, 6, 48)
    assert out.indices is None and out.locations is None and out.dots is None
    with pytest.raises(RuntimeError, match='out'):
        cuda.look(c.scenery, cams, agents=c.agents, fields=('screen',), out=out)
    ptrs = [getattr(out, k).data_ptr() for k in fields]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert cuda.look(c.scenery, cams.update(), agents=c.agents, fields=fields, out=out) is out
    torch.cuda.current_stream().wait_stream(side)
    assert [getattr(out, k).data_ptr() for k in fields] == ptrs
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cuda.look(c.scenery, cams.update(), agents=c.agents, fields=fields, out=out)
    rng = np.random.RandomState(2)
    for _ in range(3):
        util.random_velocities(c, rng)
        cuda.physics(c.scenery, c.agents)                                   # (the agents move: the graph reads their poses anew)
        g.replay()
        eager = cuda.look(c.scenery, cuda.mounted(c.agents, [[0., 0., 0.], [-.02, 0., 180.]], 48, 100.), agents=c.agents, fields=fields)
        for k in fields:
            assert np.array_equal(_bits(getattr(out, k)), _bits(getattr(eager, k))), k
        # the front cameras are the render's middle
        assert bool((out.distances < float('inf')).any())


def test_the_cameras_module_pools_what_look_sees():
    from megastep_amd import cuda, modules
    c = S.triangle_world(5, 64, 36, 'cuda')
    mounts = [[0., 0., 0.], [0., 0., 120.], [-.03, 0., -120.]]
    eyes = modules.Cameras(c, mounts, 64, 110., subsample=4, max_depth=8.)
    assert eyes.space.shape == (3, 3, 3, 16) and eyes.depth_space.shape == (3, 1, 3, 16)
    obs = eyes()
    assert obs.rgb.shape == (5, 3, 3, 3, 16) and obs.d.shape == (5, 3, 1, 3, 16)
    seen = cuda.look(c.scenery, cuda.mounted(c.agents, mounts, 64, 110.), agents=c.agents)
    rgb = seen.screen.view(5, 3, 3, 16, 4, 3).mean(4).permute(0, 1, 4, 2, 3)
    d = (1 - ((seen.distances.view(5, 3, 3, 16, 4) - c.agent_radius)/8.).clamp(0, 1)).mean(-1).unsqueeze(2)
    assert torch.allclose(obs.rgb, rgb, rtol=0, atol=1e-6) and torch.allclose(obs.d, d, rtol=0, atol=1e-6)
    assert bool((obs.rgb > 0).any()) and 0 < float(obs.d.mean()) < 1
    again = eyes()
    assert again.rgb.data_ptr() != 0 and eyes._look is not None and torch.equal(again.rgb, obs.rgb)
    around = modules.Panorama(c, res=64, subsample=4)()
    assert around.rgb.shape == (5, 3, 3, 1, 16) and around.d.shape == (5, 3, 1, 1, 16)


def test_pointgoal_with_a_panorama_graphed_is_the_eager_env_and_the_default_env_is_unchanged():
    from megastep_amd import cubicasa, graphs
    from megastep_amd.demo.envs.pointgoal import PointGoal
    from tests.test_gpu_envs import _decision
    geometries = cubicasa.sample(64, n_unique=16, seed=3)

    def make(**kw):
        torch.manual_seed(7); np.random.seed(7)
        return PointGoal(64, geometries=geometries, max_lifespan=10**6, **kw)      # (lifespans out of reach: no step draws random numbers)

    plain = make()
    assert sorted(plain.reset().obs.keys()) == ['d', 'goal', 'rgb'] and sorted(plain.obs_space.keys()) == ['d', 'goal', 'rgb']
    eager, inner = make(panorama=True), make(panorama=True)
    assert sorted(eager.obs_space.keys()) == ['d', 'goal', 'pano_d', 'pano_rgb', 'rgb']
    assert eager.obs_space.pano_rgb.shape == (1, 3, 1, 64) and eager.obs_space.pano_d.shape == (1, 1, 1, 64)
    graphed = graphs.GraphedStep(inner, warmup=2)
    first = eager.reset()
    graphed.reset()
    assert first.obs.pano_rgb.shape == (64, 1, 3, 1, 64) and first.obs.pano_d.shape == (64, 1, 1, 1, 64)
    torch.manual_seed(11)
    decisions = [_decision(eager, 64) for _ in range(5)]
    for _ in range(2):                                                       # (the graphed env's warm-up steps, eagerly)
        eager.step(decisions[0])
    for k, decision in enumerate(decisions):
        want, got = eager.step(decision), graphed.step(decision)
        for key in ('rgb', 'd', 'goal', 'pano_rgb', 'pano_d'):
            assert np.array_equal(_bits(got.obs[key]), _bits(want.obs[key])), (k, key)
        assert torch.equal(got.reward, want.reward) and torch.equal(got.reset, want.reset)
    assert bool((want.obs.pano_rgb > 0).any())
