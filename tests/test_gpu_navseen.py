"""Seen maps on the GPU: `SeenMaps.mark` equal to the numpy statement of the contract (tests/test_navseen_host.seen_rule) - maps,
gained and totals, exactly - on the distances of real `cuda.render` frames, with a map per agent and with one shared by an
env's agents; a large plan; reset masks, skipped viewers, NaN inputs, an env without cells, a grid of more than 64 KiB of
bits, `out=`, streams and graph capture; `mark_render`; and the `FloorCoverage` env, eager and as one HIP graph."""
import numpy as np
import pytest
import torch

from tests import util
from tests.test_navfield_host import CELL, RADIUS, F, plans
from tests.test_navseen_host import seen_rule

pytestmark = pytest.mark.gpu


def _core(geoms, n_agents, res, seed=0):
    from megastep_amd import core, scene
    sc = scene.scenery(geoms, n_agents, device='cuda', random=np.random.RandomState(seed))
    c = core.Core(sc, res=res, fov=130, fps=10)
    util.spawn(c, geoms, seed=seed)
    return c


def _frame(c):
    """(origins, dirs, distances) of a render of the agents as they stand: device tensors."""
    from megastep_amd import cuda
    r = cuda.render(c.scenery, c.agents, fields=('distances',))
    return c.agents.positions.clone(), cuda.camera_rays(c.agents), r.distances.clone()


def _np(t):
    return None if t is None else t.cpu().numpy()


class _Mirror:
    """seen_rule's copy of a SeenMaps: the maps and totals of every env, moved on call by call."""

    def __init__(self, maps, cell=CELL):
        grid = maps.grid
        self.cell = cell
        self.S = maps.n_maps
        self.geom = [tuple(int(v) for v in g) for g in _np(grid.geom)]
        self.countable = [_np(maps.countable)[grid.cells(e)[0]:grid.cells(e)[0] + grid.cells(e)[1]*grid.cells(e)[2]] for e in range(grid.n_envs)]
        self.maps = [np.zeros((self.S, g[3], g[2]), np.uint8) for g in self.geom]
        self.totals = np.zeros((grid.n_envs, self.S), np.int32)

    def mark(self, origins, dirs, distances, slot=None, max_range=10., reset=None):
        origins, dirs, distances, slot, reset = (_np(t) for t in (origins, dirs, distances, slot, reset))
        gained = np.zeros_like(self.totals)
        for e, geom in enumerate(self.geom):
            self.maps[e], gained[e], self.totals[e] = seen_rule.call(
                geom, self.cell, self.countable[e], self.maps[e], self.totals[e], origins[e], dirs[e], distances[e],
                slot=None if slot is None else slot[e], max_range=max_range, reset=None if reset is None else reset[e])
        return gained

    def check(self, maps, gained, want):
        assert np.array_equal(_np(gained), want), (_np(gained), want)
        assert np.array_equal(_np(maps.totals), self.totals)
        for e in range(len(self.geom)):
            for s in range(self.S):
                got = _np(maps.image(e, s))
                assert np.array_equal(got, self.maps[e][s].astype(bool)), (e, s, int((got != self.maps[e][s].astype(bool)).sum()))


_SIX = {}


def _six():
    """The six plans (three plain, three oblique), two agents each, 64 rays, and two frames of them - shared by the tests."""
    if not _SIX:
        geoms = plans(3) + plans(3, oblique=True)
        c = _core(geoms, 2, 64)
        first = _frame(c)
        c.agents.angles[:] = c.agents.angles + 100.
        c.agents.positions[:, 1] = c.agents.positions[:, 0] + torch.tensor([.3, .2], device='cuda')
        c.agents.angles[:, 1] = c.agents.angles[:, 0] + 20.              # (side by side: the two see much the same)
        _SIX.update(core=c, geoms=geoms, frames=(first, _frame(c)))
    return _SIX


@pytest.mark.parametrize('shared', [False, True])
def test_mark_is_the_rules_bits_on_rendered_frames(shared):
    from megastep_amd import cuda
    w = _six()
    grid = cuda.nav_grid(w['core'].scenery, clearance=RADIUS)
    maps = cuda.seen_maps(grid, 1 if shared else 2)
    mirror = _Mirror(maps)
    slot = torch.zeros((6, 2), dtype=torch.int64, device='cuda') if shared else None
    total = 0
    for frame in w['frames']:
        gained = maps.mark(*frame, slot=slot)
        want = mirror.mark(*frame, slot=slot)
        mirror.check(maps, gained, want)
        total += int(want.sum())
        assert (want.sum(1) > 0).all()
    assert total > 3000 and torch.isfinite(w['frames'][0][2]).any()
    if shared:
        # two viewers of one map: what both see counts once
        own = _Mirror(cuda.seen_maps(grid, 2))
        apart = own.mark(*w['frames'][1])
        again = _Mirror(maps)
        together = again.mark(*w['frames'][1], slot=slot)
        assert (together[:, 0] < apart.sum(1)).any() and (together[:, 0] >= apart.max(1)).all()
    fraction = _np(maps.fraction())
    assert np.array_equal(fraction, (mirror.totals.astype(F)/np.maximum(_np(maps.n_countable), 1)[:, None].astype(F)))
    assert (fraction > 0).all() and (fraction < 1).all()


def test_a_large_plan_with_many_words_a_lane_and_rays_cut_by_max_range():
    from megastep_amd import cuda
    geoms = plans(1, large=True)
    c = _core(geoms, 2, 256, seed=3)
    grid = cuda.nav_grid(c.scenery, clearance=RADIUS)
    assert grid.n_cells > 32*256*4                                       # (more than four words of the bitmask per lane)
    maps = cuda.seen_maps(grid, 2)
    mirror = _Mirror(maps)
    frame = _frame(c)
    assert (frame[2] > 1.5).float().mean() > .5                          # (most rays are cut at 1.5 m)
    for max_range in (1.5, 10.):
        gained = maps.mark(*frame, max_range=max_range)
        mirror.check(maps, gained, mirror.mark(*frame, max_range=max_range))
    assert (mirror.totals > 0).all() and mirror.totals.sum() > 300


def _by_hand(geoms_and_free, device='cuda', cell=CELL, clearance=RADIUS):
    """A NavGrid laid out by hand: [(geom, free (ny, nx) bool)] per env."""
    from megastep_amd import cuda
    geom = np.array([g for g, _ in geoms_and_free], np.int32)
    starts = np.concatenate([[0], np.cumsum(geom[:, 2].astype(np.int64)*geom[:, 3])]).astype(np.int64)
    free = np.concatenate([f.reshape(-1).astype(np.uint8) for _, f in geoms_and_free] + [np.zeros(1, np.uint8)])
    dev = lambda a: torch.as_tensor(a, device=device)
    return cuda.NavGrid(dev(geom), dev(starts), dev(free), cell, clearance, geom, starts)


def _fans(rng, centres, R, reach, device='cuda'):
    """(origins (N, P, 2), dirs (N, P, R, 2), distances (N, P, R)) made up: fans of R rays round `centres` (N, P, 2)."""
    n, p = centres.shape[:2]
    angle = rng.uniform(0, 2*np.pi, (n, p, 1)) + np.linspace(0, 2., R)[None, None]
    dirs = (np.stack([np.cos(angle), np.sin(angle)], -1)*rng.uniform(.5, 2., (n, p, R, 1))).astype(F)
    distances = rng.uniform(.1, reach, (n, p, R)).astype(F)
    return tuple(torch.as_tensor(a, device=device) for a in (centres.astype(F), dirs, distances))


def _odd_grid(device='cuda'):
    checker = (np.indices((40, 56)).sum(0) % 3 > 0)
    return _by_hand([((-7, 3, 56, 40), checker), ((0, 0, 0, 0), np.zeros((0, 0), bool)), ((5, -20, 31, 33), np.ones((33, 31), bool)),
                     ((-400, -400, 800, 801), np.ones((801, 800), bool))], device)            # (the last: 80 100 bytes of bits)


def _odd_calls(device='cuda'):
    """Four calls' arguments: (origins, dirs, distances, slot, reset, max_range)."""
    rng = np.random.RandomState(9)
    centres = np.array([[[-.3, 2.], [3., 3.], [1., 4.4]], [[0., 0.], [1., 1.], [2., 2.]], [[2., -1.], [3., 0.], [4.4, 1.5]],
                        [[0., 0.], [-49., 49.], [49.9, -49.9]]])
    for trial in range(4):
        origins, dirs, distances = _fans(rng, centres + rng.uniform(-.2, .2, centres.shape), 33, 6. if trial else 60., device)
        slot = torch.as_tensor(rng.randint(-1, 3, (4, 3)), device=device)                  # (-1 and 2: nobody's map)
        reset = torch.as_tensor(rng.rand(4, 2) < .4, device=device) if trial else None
        if trial == 2:
            distances[:, :, ::5] = float('nan'); distances[:, :, 1::7] = float('inf'); distances[:, 0, 2] = 0.; distances[:, 1, 3] = -2.
            dirs[:, 1, 4] = float('nan'); dirs[:, 2, 6, 1] = float('inf'); dirs[:, 0, 8] = 0.
            origins[2, 1, 0] = float('nan'); origins[0, 2] = float('-inf')
        yield origins, dirs, distances, slot, reset, 80. if trial == 0 else 10.


def test_resets_skipped_viewers_nans_an_env_without_cells_and_a_grid_of_more_than_64_kib_of_bits():
    from megastep_amd import cuda
    maps = cuda.seen_maps(_odd_grid(), 2)
    mirror = _Mirror(maps)
    for origins, dirs, distances, slot, reset, max_range in _odd_calls():
        gained = maps.mark(origins, dirs, distances, slot=slot, reset=reset, max_range=max_range)
        want = mirror.mark(origins, dirs, distances, slot=slot, reset=reset, max_range=max_range)
        mirror.check(maps, gained, want)
        assert want[1].tolist() == [0, 0] and want[0].sum() + want[2].sum() > 0 and want[3].sum() > 0
    assert mirror.totals[3].sum() > 500


def test_out_a_side_stream_and_a_graph_replayed_three_times():
    from megastep_amd import cuda
    w = _six()
    grid = cuda.nav_grid(w['core'].scenery, clearance=RADIUS)
    origins, dirs, distances = (t.clone() for t in w['frames'][0])
    maps = cuda.seen_maps(grid, 2)
    mirror = _Mirror(maps)
    out = torch.full((6, 2), -5, dtype=torch.int32, device='cuda')
    assert maps.mark(origins, dirs, distances, out=out) is out
    mirror.check(maps, out, mirror.mark(origins, dirs, distances))
    with pytest.raises(RuntimeError, match='out'):
        maps.mark(origins, dirs, distances, out=torch.zeros((6, 2), device='cuda'))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        there = maps.mark(*w['frames'][1], max_range=3.)
    side.synchronize()
    mirror.check(maps, there, mirror.mark(*w['frames'][1], max_range=3.))
    # captured once, replayed three times on inputs changed in place
    reset = torch.zeros((6, 2), dtype=torch.bool, device='cuda')
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        warm = cuda.seen_maps(grid, 2)
        warm.mark(origins, dirs, distances, reset=reset, out=torch.empty_like(out))
    torch.cuda.current_stream().wait_stream(side)
    with torch.cuda.graph(graph):
        gained = maps.mark(origins, dirs, distances, reset=reset, out=out)
    rng = np.random.RandomState(2)
    for trial in range(3):
        frame = w['frames'][trial % 2]
        origins.copy_(frame[0] + torch.as_tensor(rng.uniform(-.1, .1, (6, 2, 2)).astype(F), device='cuda'))
        dirs.copy_(frame[1]); distances.copy_(frame[2])
        reset.copy_(torch.as_tensor(rng.rand(6, 2) < .5, device='cuda'))
        graph.replay()
        want = mirror.mark(origins, dirs, distances, reset=reset)
        mirror.check(maps, gained, want)
        assert want.sum() > 0


def test_mark_render_is_mark_on_the_camera_rays_and_the_frames_distances():
    from megastep_amd import cuda, modules
    w = _six()
    c = w['core']
    grid = cuda.nav_grid(c.scenery, clearance=RADIUS)
    a, b, d = cuda.seen_maps(grid, 2), cuda.seen_maps(grid, 2), cuda.seen_maps(grid, 2)
    raw = cuda.render(c.scenery, c.agents, fields=('distances',))
    got = a.mark_render(c.agents, raw, max_range=4.)
    want = b.mark(c.agents.positions, cuda.camera_rays(c.agents), raw.distances, max_range=4.)
    framed = d.mark_render(c.agents, modules.render(c, fields=('distances',)), max_range=4.)
    assert torch.equal(got, want) and torch.equal(framed, want) and (want > 0).all()
    assert torch.equal(a.values, b.values) and torch.equal(d.values, b.values) and torch.equal(a.totals, b.totals)
    with pytest.raises(RuntimeError, match='distances'):
        a.mark_render(c.agents, cuda.render(c.scenery, c.agents, fields=('indices',)))
    # modules.Coverage: a map each, and one map for both - each agent is then paid the map's whole gain
    cover, both = modules.Coverage(c, grid, max_range=4.), modules.Coverage(c, grid, max_range=4., shared=True)
    frame = modules.render(c, fields=('distances',))
    area = cover(frame)
    assert area.shape == (6, 2) and torch.equal(area, want.float()*CELL*CELL)
    together = both(frame, reset=torch.zeros((6, 2), dtype=torch.bool, device='cuda'))
    assert together.shape == (6, 2) and torch.equal(together[:, 0], together[:, 1]) and (together[:, 0] >= area.max(1).values).all()
    assert cover.observation().shape == (6, 2, 1) and both.observation().shape == (6, 2, 1)
    assert torch.equal(cover.observation()[..., 0], b.fraction())
    assert cover.state(2).shape == (2,) + tuple(b.image(2).shape) and torch.equal(cover.state(2)[1], b.image(2, 1)) and both.state(2).shape[0] == 1


def _actions(rng, n, a):
    return torch.as_tensor(rng.randint(0, 7, (n, a)), device='cuda')


def test_floor_coverage_pays_for_every_countable_cell_once_an_episode():
    """FloorCoverage(8), 40 steps of random actions: per agent and episode the rewards sum to the map's total, which is the
    number of countable cells its image holds; totals never fall inside an episode, and start from what the first frame gained."""
    from megastep_amd import arrdict
    from megastep_amd.demo import FloorCoverage
    torch.manual_seed(5); np.random.seed(5)
    env = FloorCoverage(8, n_agents=2, geometries=plans(8), max_lifespan=24)
    assert env.obs_space.coverage.shape == (2, 1) and env.obs_space.rgb.shape == (2, 3, 1, 64)
    grid, maps = env.grid, env.maps
    countable = [_np(maps.countable)[grid.cells(e)[0]:grid.cells(e)[0] + grid.cells(e)[1]*grid.cells(e)[2]].astype(bool) for e in range(8)]
    for e in range(8):
        free = _np(grid.image(e)).reshape(-1)
        assert (countable[e] <= free).all() and 500 < countable[e].sum() == int(maps.n_countable[e])
    assert sum(c.sum() for c in countable) < int(grid.free.sum())        # (free cells outside the building, or shut in, do not count)
    rng = np.random.RandomState(6)
    world = env.reset()
    assert world.reset.all() and world.obs.coverage.shape == (8, 2, 1)
    cells = np.zeros((8, 2))                                             # reward/c^2 summed over the episode so far
    before = np.zeros((8, 2), np.int64)
    starts, started = 0, np.ones((8, 2), bool)
    for t in range(41):
        if t:
            started = _np(env._over)                                     # who starts over at this step
            world = env.step(arrdict.arrdict(actions=_actions(rng, 8, 2)))
            assert np.array_equal(_np(world.reset), started.any(1))
            starts += int(started.sum())
        gained = _np(world.reward).astype(np.float64)/(CELL*CELL)
        assert (gained == np.round(gained)).all() and (gained >= 0).all()
        cells = np.where(started, 0., cells) + gained
        totals = _np(maps.totals)
        assert np.array_equal(cells, totals)
        assert np.array_equal(totals[started], gained[started])
        assert (totals[~started] >= before[~started]).all()
        for e in range(8):
            for a in range(2):
                assert totals[e, a] == (_np(maps.image(e, a)).reshape(-1) & countable[e]).sum()
        assert np.array_equal(_np(world.obs.coverage)[..., 0], _np(maps.fraction()))
        before = totals
    assert starts > 8 and before.sum() > 100
    state = env.state(0)
    assert state.seen.shape == (2,) + tuple(maps.image(0).shape) and state.fraction.shape == (2,)


def test_floor_coverage_as_a_hip_graph_equals_the_eager_env():
    from megastep_amd import arrdict, graphs
    from megastep_amd.demo import FloorCoverage
    rng = np.random.RandomState(8)
    acts = [_actions(rng, 8, 1) for _ in range(8)]
    logs = []
    for graphed in (False, True):
        torch.manual_seed(3); np.random.seed(3)
        env = FloorCoverage(8, geometries=plans(8), max_lifespan=10**6, complete=.05)
        stepper = graphs.GraphedStep(env, warmup=3) if graphed else env
        stepper.reset()
        log = []
        # the graphed env's first step call is four steps under its actions: three of warm-up and the captured one
        for a in (acts if graphed else [acts[0]]*3 + acts):
            world = stepper.step(arrdict.arrdict(actions=a))
            log.append((world.reward.clone(), world.reset.clone(), env.maps.totals.clone()))
        logs.append(log)
    eager, graphed = logs
    for k in range(8):
        for got, want in zip(graphed[k], eager[k + 3]):
            assert torch.equal(got, want), k
    assert sum(float(r.sum()) for r, _, _ in graphed) > 0
    assert any(bool(reset.any()) for _, reset, _ in graphed[1:])         # somebody had seen enough and started over inside the graph
