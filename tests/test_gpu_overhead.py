"""Top-down pictures on the GPU (`cuda.overhead`, `scene.display`, `modules.Overhead`): the kernel gives the binary32 numpy
rule (tests/test_overhead_host.py) bit for bit - colours and line indices, aligned and oblique plans, rotated and mirrored
views, sizes that are not multiples of the tile, several views per image, env subsets - draws the agents as the render
does without writing the scenery, culls without changing a bit (a plan too large for one LDS list included), reuses
buffers and replays in a HIP graph."""
import numpy as np
import pytest
import torch

from tests import util
from tests.test_gpu_parity import _world
from tests.test_overhead_host import overhead_rule

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.detach().cpu().numpy().view(np.int32)


def _views(c, envs, n_views, height, width, rng, oblique=True):
    """(K, V, 6) views about random points of each image's env: rotated (if `oblique`), mirrored now and then, at 2-10 cm a pixel."""
    sc = c.scenery
    af = sc.n_agents*sc.model.shape[0]
    out = np.zeros((len(envs), n_views, 6), np.float32)
    for k, e in enumerate(envs):
        walls = sc.lines[int(e) % len(sc.lines)][af:].cpu().numpy().reshape(-1, 2)
        lo, hi = walls.min(0), walls.max(0)
        for v in range(n_views):
            a = rng.uniform(0, 2*np.pi) if oblique else 0.
            s = rng.uniform(.02, .1)
            m = rng.choice([-1., 1.]) if oblique else -1.
            centre = lo + rng.uniform(0, 1, 2)*(hi - lo)
            g = np.array([s*np.cos(a), -m*s*np.sin(a), 0, s*np.sin(a), m*s*np.cos(a), 0])
            g[2] = centre[0] - g[0]*width/2 - g[1]*height/2
            g[5] = centre[1] - g[3]*width/2 - g[4]*height/2
            out[k, v] = g
    return torch.as_tensor(out, device='cuda')


def _expect(c, views, height, width, envs, half_width=.05, lit=True, background=None):
    """The numpy rule for every image and view, over the lines as the scenery holds them now."""
    from megastep_amd import cuda
    background = cuda.OVERHEAD_BACKGROUND if background is None else background
    sc = c.scenery
    af = sc.n_agents*sc.model.shape[0]
    lines = sc.lines.vals.cpu().numpy()
    starts, widths = sc.lines.starts.cpu().numpy(), sc.lines.widths.cpu().numpy()
    tw, ts = sc.textures.widths.cpu().numpy(), sc.textures.starts.cpu().numpy()
    texels, baked = sc.textures.vals.cpu().numpy(), sc.baked.vals.cpu().numpy()
    views = views.cpu().numpy()
    K, V = views.shape[:2]
    rgb = np.zeros((K, V, 3, height, width), np.float32)
    idx = np.zeros((K, V, height, width), np.int32)
    for k, e in enumerate(envs):
        for v in range(V):
            if not 0 <= e < len(widths):
                rgb[k, v] = np.asarray(background, np.float32)[:, None, None]
                idx[k, v] = -1
                continue
            s, L = starts[e], widths[e]
            rgb[k, v], idx[k, v] = overhead_rule(lines[s:s + L], views[k, v], height, width, half_width, af,
                                                 (tw[s:s + L], ts[s:s + L], texels, baked), lit, background)
    return rgb, idx


def _assert_rule(c, r, views, height, width, envs, **kw):
    rgb, idx = _expect(c, views, height, width, envs, **kw)
    if r.indices is not None:
        assert np.array_equal(r.indices.cpu().numpy(), idx)
        assert (idx >= 0).mean() > .01                  # (something was drawn)
    if r.rgb is not None:
        assert np.array_equal(_bits(r.rgb), rgb.view(np.int32))


def _moved(c, seed):
    from megastep_amd import cuda
    util.random_velocities(c, np.random.RandomState(seed))
    cuda.physics(c.scenery, c.agents)


@pytest.mark.parametrize('toy,n_agents,size,lit', [('box', 1, (37, 53), True), ('column', 4, (48, 32), False),
                                                   (None, 1, (37, 53), True), (None, 4, (64, 17), True), ('oblique', 4, (37, 53), False)])
def test_the_kernel_is_the_numpy_rule(toy, n_agents, size, lit):
    from megastep_amd import core, cubicasa, cuda, scene
    if toy == 'oblique':
        np.random.seed(2)
        geoms = cubicasa.sample(5, n_unique=32, seed=5, oblique=True)
        c = core.Core(scene.scenery(geoms, n_agents, device='cuda', random=np.random.RandomState(2)), res=64, fov=130, fps=10)
        util.spawn(c, geoms, seed=6)
    else:
        c, _ = _world(5, n_agents, 64, 130, seed=3, toy=toy)
    _moved(c, 1)
    cuda.render(c.scenery, c.agents, fields=('distances',))               # (draws the agents into `lines` for the numpy rule)
    rng = np.random.RandomState(4)
    h, w = size
    views = _views(c, range(5), 2, h, w, rng)
    r = cuda.overhead(c.scenery, views, size, agents=c.agents, lit=lit, half_width=.06)
    assert r.rgb.shape == (5, 2, 3, h, w) and r.indices.shape == (5, 2, h, w)
    _assert_rule(c, r, views, h, w, range(5), lit=lit, half_width=.06)
    if n_agents > 1:                                    # views on the agents themselves: their bodies are drawn
        views = cuda.agent_views(c.agents, size, 1.)
        r = cuda.overhead(c.scenery, views, size, agents=c.agents, lit=lit)
        _assert_rule(c, r, views, h, w, range(5), lit=lit)
        af = n_agents*c.scenery.model.shape[0]
        assert ((r.indices >= 0) & (r.indices < af)).any()


def test_fields_alone_env_subsets_and_ids_out_of_range():
    from megastep_amd import cuda
    c, _ = _world(6, 2, 64, 130, seed=5)
    _moved(c, 2)
    cuda.render(c.scenery, c.agents, fields=('distances',))
    rng = np.random.RandomState(5)
    envs = [4, 1, 4, 6, 0, -1, 1]                      # repeats, and two ids out of range
    views = _views(c, envs, 3, 40, 24, rng)
    e = torch.tensor(envs, dtype=torch.int32, device='cuda')
    both = cuda.overhead(c.scenery, views, (40, 24), agents=c.agents, envs=e, background=(.1, .2, .3))
    _assert_rule(c, both, views, 40, 24, envs, background=(.1, .2, .3))
    for k in (3, 5):
        assert (both.indices[k] == -1).all()
        assert torch.equal(both.rgb[k], torch.tensor([.1, .2, .3], device='cuda')[None, :, None, None].expand(3, 3, 40, 24))
    rgb = cuda.overhead(c.scenery, views, (40, 24), agents=c.agents, envs=e.long(), background=(.1, .2, .3), fields=('rgb',))
    idx = cuda.overhead(c.scenery, views, (40, 24), agents=c.agents, envs=e, fields=('indices',))
    assert rgb.indices is None and idx.rgb is None
    assert torch.equal(_t(rgb.rgb), _t(both.rgb)) and torch.equal(idx.indices, both.indices)
    same = cuda.overhead(c.scenery, views[[0, 0]].contiguous(), (40, 24), agents=c.agents, envs=e[[0, 2]].contiguous())
    assert torch.equal(_t(same.rgb[0]), _t(same.rgb[1]))


def _t(x):
    return x.view(torch.int32)


def test_drawn_agents_are_the_rendered_rows_and_nothing_is_written():
    from megastep_amd import cuda
    c, _ = _world(4, 4, 64, 130, seed=7)
    rng = np.random.RandomState(7)
    views = _views(c, range(4), 1, 64, 64, rng)
    for step in range(3):
        _moved(c, 10 + step)
        before = c.scenery.lines.vals.clone()
        drawn = cuda.overhead(c.scenery, views, 64, agents=c.agents)
        assert torch.equal(_t(c.scenery.lines.vals), _t(before))           # nothing written
        cuda.render(c.scenery, c.agents, fields=('distances',))
        stored = cuda.overhead(c.scenery, views, 64)
        assert torch.equal(drawn.indices, stored.indices) and torch.equal(_t(drawn.rgb), _t(stored.rgb))
    ag = cuda.agent_views(c.agents, 32, 1.)
    assert torch.equal(cuda.overhead(c.scenery, ag, 32, agents=c.agents).indices, cuda.overhead(c.scenery, ag, 32).indices)


def _plan_with_walls(n_walls, seed):
    rng = np.random.RandomState(seed)
    a = rng.uniform(1, 11, (n_walls, 2))
    d = rng.normal(size=(n_walls, 2))*.3
    return dict(walls=np.stack([a, a + d], 1), lights=np.array([[6., 6.], [3., 9.]]))


@pytest.mark.parametrize('whole', [False, True])
def test_the_cull_changes_no_bit(whole):
    """Cull on and off (ms_debug_overhead_cull) give the same bits: zoomed-in views, and - `whole` - views of a 2000-wall
    plan seen whole in 16 x 16 images, so that every line of the plan survives one tile's cull and the list runs over
    several LDS chunks."""
    from megastep_amd import _lib, core, cuda, scene
    if whole:
        np.random.seed(0)
        geoms = [_plan_with_walls(2000, 1), _plan_with_walls(1500, 2)]
        c = core.Core(scene.scenery(geoms, 2, device='cuda', random=np.random.RandomState(0)), res=64, fov=130, fps=10)
        c.agents.positions[:] = torch.tensor([6., 6.], device='cuda')
        views = cuda.plan_views(c.scenery, 16)
        size = 16
    else:
        c, _ = _world(6, 3, 64, 130, seed=9, toy=None)
        views = _views(c, range(6), 2, 45, 70, np.random.RandomState(9))
        size = (45, 70)
    h = _lib.lib()
    try:
        on = cuda.overhead(c.scenery, views, size, agents=c.agents)
        h.ms_debug_overhead_cull(0)
        off = cuda.overhead(c.scenery, views, size, agents=c.agents)
    finally:
        h.ms_debug_overhead_cull(1)
    assert torch.equal(on.indices, off.indices) and torch.equal(_t(on.rgb), _t(off.rgb))
    if whole:
        cuda.render(c.scenery, c.agents, fields=('distances',))
        _assert_rule(c, on, views, 16, 16, range(2))


def test_out_reuse_and_a_graph_replay_give_what_eager_calls_give():
    from megastep_amd import cuda
    c, _ = _world(6, 2, 64, 130, seed=17)
    views = cuda.agent_views(c.agents, 32, 4.)
    out = cuda.overhead(c.scenery, views, 32, agents=c.agents)
    again = cuda.overhead(c.scenery, views, 32, agents=c.agents, out=out)
    assert again is out
    with pytest.raises(RuntimeError, match='out'):
        cuda.overhead(c.scenery, views, 32, agents=c.agents, out=out, fields=('rgb',))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        views.copy_(cuda.agent_views(c.agents, 32, 4.))
        cuda.overhead(c.scenery, views, 32, agents=c.agents, out=out)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        views.copy_(cuda.agent_views(c.agents, 32, 4.))
        cuda.overhead(c.scenery, views, 32, agents=c.agents, out=out)
    for step in range(3):
        _moved(c, 20 + step)
        g.replay()
        eager = cuda.overhead(c.scenery, cuda.agent_views(c.agents, 32, 4.), 32, agents=c.agents)
        assert torch.equal(out.indices, eager.indices) and torch.equal(_t(out.rgb), _t(eager.rgb))


def test_the_overhead_module_shows_each_agent_at_its_centre():
    from megastep_amd import cuda, modules
    from megastep_amd import geometry
    c, _ = _world(5, 3, 64, 130, seed=21, toy='box')       # (agents well apart and a metre from the walls: nothing else is as near)
    spots = torch.tensor([[1.5, 1.5], [2.5, 3.5], [3.5, 1.5]], device='cuda') + geometry.MARGIN
    c.agents.positions[:] = spots + torch.rand(5, 3, 2, device='cuda')*.2
    c.agents.angles[:] = torch.rand(5, 3, device='cuda')*360 - 180
    m = modules.Overhead(c, size=32, radius=4.)
    obs = m()
    assert tuple(obs.shape) == (5,) + m.space.shape == (5, 3, 3, 32, 32)
    assert m.state(2).shape == (3, 3, 32, 32)
    r = cuda.overhead(c.scenery, m.views(), 32, agents=c.agents, half_width=m.half_width)
    assert torch.equal(_t(r.rgb), _t(obs))
    M = c.scenery.model.shape[0]
    centre = r.indices[:, :, 15:17, 15:17].reshape(5, 3, 4)
    own = torch.arange(3, device='cuda')[None, :, None]
    assert ((centre >= 0) & (centre // M == own)).all()
    ptr = obs.data_ptr()
    c.agents.angles[:] += 30.
    assert m().data_ptr() == ptr                                         # (the buffers are reused)


def test_display_is_a_picture_of_the_env_with_its_light():
    from megastep_amd import scene, toys
    c, _ = _world(2, 1, 64, 130, seed=0, toy='box')
    img = scene.display(c.scenery, 1, size=128)
    assert img.dtype == np.uint8 and img.shape == (128, 128, 3)
    middle = toys.box()['lights'][0]                        # the box's one light, in the middle of the image
    from megastep_amd import cuda
    g = cuda.plan_views(c.scenery, 128, envs=[1])[0, 0].cpu().numpy()
    j, i = int((middle[0] - g[2])/g[0]), int((middle[1] - g[5])/g[4])
    r, gr, b = (int(v) for v in img[i, j])
    assert r > 200 and gr > 200 and b < 100                 # yellow
    assert len({tuple(p) for p in img.reshape(-1, 3)}) > 10  # walls in their colours around it


def test_more_than_two_to_the_31_colour_values():
    """One call whose rgb output holds more than 2^31 floats (2731 images of 512 x 512: 8.6 GB): the last image is the rule's."""
    from megastep_amd import cuda
    free, _ = torch.cuda.mem_get_info()
    if free < 16 << 30:
        pytest.skip('needs 16 GB of free device memory')
    c, _ = _world(4, 2, 64, 130, seed=23)
    K = 2731
    assert K*3*512*512 > 2**31
    envs = torch.arange(K, device='cuda', dtype=torch.int32) % 4
    views = cuda.plan_views(c.scenery, 512, envs=envs)
    r = cuda.overhead(c.scenery, views, 512, envs=envs)
    rgb, idx = _expect(c, views[-1:], 512, 512, [int(envs[-1])])
    assert np.array_equal(r.indices[-1].cpu().numpy(), idx[0])
    assert np.array_equal(_bits(r.rgb[-1]), rgb[0].view(np.int32))
    del r
