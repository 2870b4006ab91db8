"""Ray queries on the GPU (`cuda.raycast`, `cuda.camera_rays`, `cuda.line_of_sight`): the render's camera rays cast through
the query give the render's planes bit for bit; arbitrary rays give the numpy restatement of the reference's per-ray rule
(tests/test_raycast_host.py, itself checked against the oracle) bit for bit; the wall grid changes no bit and is used; the
query writes nothing; it reuses buffers and replays in a HIP graph."""
import numpy as np
import pytest
import torch

from tests import util
from tests.test_gpu_parity import _world
from tests.test_gpu_scale import _big_world
from tests.test_raycast_host import raycast_rule

pytestmark = pytest.mark.gpu

PLANES = ('indices', 'locations', 'dots', 'distances')


def _bits(t):
    return t.detach().cpu().numpy().view(np.int32)


def _camera_query(c):
    from megastep_amd import cuda
    n, a = c.agents.angles.shape
    dirs = cuda.camera_rays(c.agents)
    assert dirs.shape == (n, a, c.res, 2)
    origins = c.agents.positions[:, :, None, :].expand(n, a, c.res, 2).reshape(n, a*c.res, 2).contiguous()
    return origins, dirs.reshape(n, a*c.res, 2)


def _assert_render_equal(c, q, r):
    n, a = c.agents.angles.shape
    for k in PLANES:
        assert np.array_equal(_bits(getattr(q, k)).reshape(n, a, c.res), _bits(getattr(r, k))), k
    M = c.scenery.model.shape[0]
    idx = r.indices
    want = torch.where((idx >= 0) & (idx < a*M), idx//M, torch.full_like(idx, -1))
    assert torch.equal(q.agents.view(n, a, c.res), want)


@pytest.mark.parametrize('n_agents,res,fov,light_grid', [(1, 64, 130, True), (3, 100, 90, True), (4, 128, 70, False),
                                                         (4, 512, 70, True), (3, 64, 130, True)])
def test_camera_rays_through_the_query_are_the_render(monkeypatch, n_agents, res, fov, light_grid):
    from megastep_amd import cuda
    if not light_grid:
        monkeypatch.setattr(cuda.Scenery, 'LIGHT_GRID', False)
    c, _ = _world(6, n_agents, res, fov, seed=11)
    rng = np.random.RandomState(4)
    hits_agents = 0
    for step in range(3):
        util.random_velocities(c, rng)
        cuda.physics(c.scenery, c.agents)
        if n_agents > 1 and step == 2:                     # two agents face to face, so that rays land on an agent
            c.agents.positions[0, 1] = c.agents.positions[0, 0] + torch.tensor([.4, 0.], device='cuda')
            c.agents.angles[0, 0], c.agents.angles[0, 1] = 0., 180.
        r = cuda.render(c.scenery, c.agents)
        o, d = _camera_query(c)
        q = cuda.raycast(c.scenery, o, d, agents=c.agents)
        _assert_render_equal(c, q, r)
        hits_agents += int((q.agents >= 0).sum())
    assert (r.indices >= 0).float().mean() > .5
    if n_agents > 1:
        assert hits_agents > 0


def test_camera_rays_through_the_query_are_the_render_at_full_size():
    """4096 envs x 4 agents x 64 rays on 512 distinct plans: every plane, bit for bit, and the grid serves most rays."""
    from megastep_amd import cuda
    c, _, _ = _big_world(4096, 4, 64, 130, n_distinct=512, fast=True)
    rng = np.random.RandomState(7)
    for _ in range(2):
        util.random_velocities(c, rng)
        cuda.physics(c.scenery, c.agents)
    r = cuda.render(c.scenery, c.agents, fields=PLANES)
    o, d = _camera_query(c)
    counter = torch.zeros(1, dtype=torch.int32, device='cuda')
    q = cuda.raycast(c.scenery, o, d, agents=c.agents, grid_rays=counter)
    _assert_render_equal(c, q, r)
    assert int(counter) > .5*o.shape[0]*o.shape[1]        # (rays whose |ru|^2 rounds below 1 go without)


def _random_rays(c, rng, n_rays, clustered=0):
    """Origins: uniform over each env's walls' bounding box grown by 2 m (so some lie outside the plan), a quarter of them
    on wall endpoints; directions: random angles at lengths from 0.3 to 20, a sixth axis-aligned, a sixth within 1e-3 rad
    of a wall of the env.  The first `clustered` rays of an env come 64 from each of a few points inside the plan instead,
    at lengths from 1 to 8 - rays that share their origin's cell, as a lidar ring's do."""
    sc = c.scenery
    AF = sc.n_agents*sc.model.shape[0]
    lines = sc.lines.vals.cpu().numpy()
    starts, widths = sc.lines.starts.cpu().numpy(), sc.lines.widths.cpu().numpy()
    n = len(widths)
    o = np.zeros((n, n_rays, 2), np.float32)
    d = np.zeros((n, n_rays, 2), np.float32)
    for e in range(n):
        walls = lines[starts[e] + AF:starts[e] + widths[e]]
        pts = walls.reshape(-1, 2)
        lo, hi = pts.min(0) - 2, pts.max(0) + 2
        o[e] = rng.uniform(lo, hi, (n_rays, 2))
        k = rng.rand(n_rays) < .25
        o[e][k] = pts[rng.randint(len(pts), size=k.sum())]
        ang = rng.uniform(-np.pi, np.pi, n_rays)
        length = rng.choice([.3, .9, 1., 1.5, 3., 7.9, 8., 8.5, 20.], n_rays)
        kind = rng.randint(6, size=n_rays)
        ang = np.where(kind == 0, rng.randint(4, size=n_rays)*np.pi/2, ang)
        w = walls[rng.randint(len(walls), size=n_rays)]
        along = np.arctan2(w[:, 1, 1] - w[:, 0, 1], w[:, 1, 0] - w[:, 0, 0]) + rng.uniform(-1e-3, 1e-3, n_rays)
        ang = np.where(kind == 1, along, ang)
        d[e] = np.stack([length*np.cos(ang), length*np.sin(ang)], -1)
        for k0 in range(0, clustered, 64):
            o[e, k0:k0 + 64] = rng.uniform(lo + 2, hi - 2, 2)
            d[e, k0:k0 + 64] *= (rng.uniform(1, 8, 64)/length[k0:k0 + 64])[:, None]
    dev = sc.lines.vals.device
    return torch.as_tensor(o, device=dev), torch.as_tensor(d, device=dev)


def _assert_rule(c, o, d, q, envs, near, with_agents):
    sc = c.scenery
    AF = sc.n_agents*sc.model.shape[0]
    lines = sc.lines.vals.cpu().numpy()
    starts, widths = sc.lines.starts.cpu().numpy(), sc.lines.widths.cpu().numpy()
    for e in envs:
        rows = lines[starts[e]:starts[e] + widths[e]].copy()
        if not with_agents:
            rows[:AF] = np.nan                                # (NaN rows never hit: the static walls alone, indices kept)
        want = raycast_rule(rows, o[e].cpu().numpy(), d[e].cpu().numpy(), near)
        for k in PLANES:
            assert np.array_equal(_bits(getattr(q, k)[e]), want[k].view(np.int32)), (e, k)


@pytest.mark.parametrize('oblique', [False, True])
def test_arbitrary_rays_follow_the_rule(oblique):
    from megastep_amd import core, cubicasa, cuda, scene
    np.random.seed(2)
    geometries = cubicasa.sample(12, n_unique=32, seed=5, oblique=oblique)
    sc = scene.scenery(geometries, 3, device='cuda', random=np.random.RandomState(2))
    c = core.Core(sc, res=64, fov=130, fps=10)
    util.spawn(c, geometries, seed=6)
    rng = np.random.RandomState(8)
    util.random_velocities(c, rng)
    cuda.physics(c.scenery, c.agents)
    cuda.render(c.scenery, c.agents, fields=('distances',))           # (draws the bodies into `lines` for the numpy rule)
    o, d = _random_rays(c, rng, 704, clustered=256)
    counter = torch.zeros(1, dtype=torch.int32, device='cuda')
    q = cuda.raycast(c.scenery, o, d, agents=c.agents, grid_rays=counter)
    _assert_rule(c, o, d, q, [0, 3, 7, 11], c.agent_radius, True)
    assert int(counter) > 0
    assert (q.indices >= 0).float().mean() > .3
    s = cuda.raycast(c.scenery, o, d, near=.05)                      # static walls only
    AF = sc.n_agents*sc.model.shape[0]
    assert not bool(((s.indices >= 0) & (s.indices < AF)).any()) and bool((s.agents == -1).all())
    _assert_rule(c, o, d, s, [1, 5, 10], .05, False)


def test_the_wall_grid_changes_no_bit_and_is_taken():
    from megastep_amd import core, cubicasa, cuda, scene
    np.random.seed(3)
    geometries = cubicasa.sample(16, n_unique=32, seed=9)
    worlds = []
    for grid in (True, False):
        sc = scene.scenery(geometries, 2, device='cuda', random=np.random.RandomState(3), bake=False)
        cuda.bake(sc, wall_grid=grid)
        c = core.Core(sc, res=64, fov=130, fps=10)
        util.spawn(c, geometries, seed=1)
        worlds.append(c)
    assert worlds[0].scenery._wg is not None and worlds[1].scenery._wg is None
    assert torch.equal(worlds[0].scenery.lines.vals, worlds[1].scenery.lines.vals)
    rng = np.random.RandomState(12)
    o, d = _random_rays(worlds[0], rng, 1024, clustered=512)
    wg_near = worlds[0].scenery._wg.near
    for near, with_agents in ((.1, True), (.1, False), (wg_near*2, True), (0., False)):
        results = []
        for c in worlds:
            counter = torch.zeros(1, dtype=torch.int32, device='cuda')
            results.append((cuda.raycast(c.scenery, o, d, agents=c.agents if with_agents else None, near=near, grid_rays=counter), int(counter)))
        (a, n_grid), (b, n_flat) = results
        for k in cuda.RAYCAST_FIELDS:
            assert np.array_equal(_bits(getattr(a, k)), _bits(getattr(b, k))), (near, k)
        assert n_flat == 0
        if near*1.001 < wg_near:
            assert n_grid > .5*16*512                       # (the clustered rays, nearly all)
        else:
            assert n_grid == 0
    _assert_rule(worlds[0], o, d, a, [0, 9, 15], 0., False)


def test_the_query_writes_nothing_and_reuses_buffers():
    from megastep_amd import cuda
    c, _ = _world(5, 3, 64, 130, seed=13)
    cuda.render(c.scenery, c.agents)
    util.random_velocities(c, np.random.RandomState(1))
    cuda.physics(c.scenery, c.agents)                                # (agents moved: the rows in `lines` are the old poses)
    before = c.scenery.lines.vals.clone()
    o, d = _random_rays(c, np.random.RandomState(2), 300)
    full = cuda.raycast(c.scenery, o, d, agents=c.agents)
    assert torch.equal(c.scenery.lines.vals.view(torch.int32), before.view(torch.int32))
    for fields in [('distances',), ('indices', 'agents'), ('locations', 'dots')]:
        part = cuda.raycast(c.scenery, o, d, agents=c.agents, fields=fields)
        for k in cuda.RAYCAST_FIELDS:
            assert (getattr(part, k) is None) == (k not in fields)
            if k in fields:
                assert np.array_equal(_bits(getattr(part, k)), _bits(getattr(full, k))), k
        again = cuda.raycast(c.scenery, o, d, agents=c.agents, fields=fields, out=part)
        assert again is part
    with pytest.raises(RuntimeError, match='out'):
        cuda.raycast(c.scenery, o, d, agents=c.agents, fields=('distances',), out=full)


def test_a_graphed_raycast_replays_what_eager_calls_give():
    from megastep_amd import cuda
    c, _ = _world(6, 2, 64, 130, seed=17)
    o, d = _camera_query(c)
    rng = np.random.RandomState(3)
    util.random_velocities(c, rng)
    out = cuda.raycast(c.scenery, o, d, agents=c.agents)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        cuda.raycast(c.scenery, o, d, agents=c.agents, out=out)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cuda.raycast(c.scenery, o, d, agents=c.agents, out=out)
    for _ in range(3):
        cuda.physics(c.scenery, c.agents)
        o.copy_(c.agents.positions[:, :, None, :].expand(6, 2, 64, 2).reshape(6, 128, 2))
        d.copy_(cuda.camera_rays(c.agents).reshape(6, 128, 2))
        g.replay()
        eager = cuda.raycast(c.scenery, o, d, agents=c.agents)
        for k in cuda.RAYCAST_FIELDS:
            assert np.array_equal(_bits(getattr(out, k)), _bits(getattr(eager, k))), k
        r = cuda.render(c.scenery, c.agents)
        _assert_render_equal(c, out, r)


def test_a_raycast_inside_a_graphed_env_step():
    """graphs.GraphedStep around an env whose step also asks a line-of-sight question: the replayed answers are the eager ones."""
    from megastep_amd import cubicasa, cuda, graphs
    from megastep_amd.demo import Deathmatch
    from tests.test_gpu_envs import _decision

    class Sighted:
        def __init__(self, env):
            self.env, self.device = env, env.device

        def reset(self):
            return self.env.reset()

        def step(self, decision):
            world = self.env.step(decision)
            c = self.env.core
            world['sees'] = cuda.line_of_sight(c.scenery, c.agents, 0, 1)
            return world

    torch.manual_seed(5); np.random.seed(5)
    inner = Deathmatch(32, 4, geometries=cubicasa.sample(8, n_unique=16))
    env = graphs.GraphedStep(Sighted(inner), warmup=2)
    env.reset()
    for _ in range(4):
        world = env.step(_decision(inner, 32))
        c = inner.core
        assert torch.equal(world['sees'], cuda.line_of_sight(c.scenery, c.agents, 0, 1))


def _los_brute(c, a, b):
    """line_of_sight by brute force in torch: every line of the env (bodies as the render draws them) against the segment a -> b."""
    from megastep_amd import cuda
    cuda.render(c.scenery, c.agents, fields=('distances',))         # (draws the bodies)
    sc = c.scenery
    n = len(sc.lines)
    M = sc.model.shape[0]
    out = torch.zeros(n, dtype=torch.bool)
    lines, starts, widths = sc.lines.vals.cpu(), sc.lines.starts.cpu(), sc.lines.widths.cpu()
    pos = c.agents.positions.cpu()
    for e in range(n):
        p, q = pos[e, a], pos[e, b]
        d = q - p
        rows = lines[starts[e]:starts[e] + widths[e]]
        want = raycast_rule(rows.numpy(), p[None].numpy(), d[None].numpy(), c.agent_radius)
        i = int(want['indices'][0])
        out[e] = (i >= 0 and i < sc.n_agents*M and i//M == b) or not (want['distances'][0] < float(torch.sqrt(d[0]*d[0] + d[1]*d[1])))
    return out


@pytest.mark.parametrize('toy', ['box', None])
def test_line_of_sight_agrees_with_brute_force(toy):
    from megastep_amd import cuda
    c, _ = _world(40, 4, 64, 130, seed=19, toy=toy)
    pairs = [(a, b) for a in range(4) for b in range(4) if a != b]
    seen = []
    for a, b in pairs:
        got = cuda.line_of_sight(c.scenery, c.agents, a, b).cpu()
        assert torch.equal(got, _los_brute(c, a, b)), (a, b)
        seen.append(got)
    seen = torch.stack(seen)
    if toy == 'box':
        assert seen.float().mean() > .5                     # (open boxes: mostly in sight)
    else:
        assert 0 < seen.float().mean() < 1                  # (floorplans: walls between some)
    # the tensor form: per env its own pair
    a = torch.zeros(40, dtype=torch.int64, device='cuda')
    b = torch.arange(40, device='cuda') % 3 + 1
    got = cuda.line_of_sight(c.scenery, c.agents, a, b).cpu()
    for e in range(0, 40, 7):
        assert bool(got[e]) == bool(seen[pairs.index((0, int(b[e])))][e])
