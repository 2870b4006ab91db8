"""Clearance on the GPU (cuda.clearance_fields, ClearanceFields.update / .nav_grid, cuda.clearance, modules.Proximity): the kernels are
held to EQUALITY with tests/test_navclear_host.py's clear_rule - values, nearest, fits, distances and towards as bits - on small
worlds, with either cull instantiation; the fits to the existing grid's free bytes; the LDS list at its boundary; masked updates;
the query with the agents' live rows; the module under graph capture; and what is built on the layer."""
import numpy as np
import pytest
import torch

from tests import util
from tests.test_navfield_host import CELL, CELLS, RADIUS, F, bits, nav_rule, plans
from tests.test_navclear_host import clear_rule, query_rule, same
from tests.test_gpu_navseen import _np
from tests.test_gpu_navwindow import _same as window_same

pytestmark = pytest.mark.gpu
QUERY = ('distances', 'nearest', 'towards')


def _rows(scenery):
    """[(L, 4) float32] per env: ALL the scenery's rows as they stand, the agents' first."""
    lines = scenery.lines
    vals, starts, widths = _np(lines.vals).reshape(-1, 4), _np(lines.starts), _np(lines.widths)
    return [vals[starts[e]:starts[e] + widths[e]] for e in range(len(widths))]


def _af(scenery):
    return scenery.n_agents*scenery.model.shape[0]


def _field(clear):
    return dict(values=_np(clear.values), nearest=_np(clear.nearest), fits=_np(clear.fits))


def _field_rule(clear, rows, af):
    """clear_rule on a mirror of what the ClearanceFields reads: (values, nearest, fits) in the stores' layouts."""
    grid, K = clear.grid, len(clear.radii)
    size = max(grid.n_cells, 1)
    out = dict(values=np.full(size, np.inf, F), nearest=np.full(size, -1, np.int32), fits=np.ones(max(K, 1)*size, np.uint8))
    for n in range(grid.n_envs):
        s, ny, nx = grid.cells(n)
        if nx*ny == 0:
            continue
        values, nearest, fits = clear_rule.field(rows[n][af:], tuple(int(v) for v in grid._host_geom[n]), grid.cell, clear.max_range, clear.radii, first=af)
        out['values'][s:s + ny*nx], out['nearest'][s:s + ny*nx] = values.reshape(-1), nearest.reshape(-1)
        for k in range(K):
            out['fits'][K*s + k*ny*nx:][:ny*nx] = fits[k].reshape(-1)
    return out


_WORLD = {}


def _world():
    """Three envs - two plans and an oblique one - of one agent: (scenery, its rows read back)."""
    if not _WORLD:
        from megastep_amd import scene
        np.random.seed(2)
        geoms = plans(2) + plans(1, oblique=True)
        sc = scene.scenery(geoms, 1, device='cuda', random=np.random.RandomState(2), bake=False)
        _WORLD.update(scenery=sc, rows=_rows(sc), geoms=geoms)
    return _WORLD


def _crowd():
    """Two envs of three agents, spawned, a physics step behind them and a render that left their drawn rows in the scenery."""
    if 'crowd' not in _WORLD:
        from megastep_amd import core, cuda, scene
        np.random.seed(3)
        geoms = plans(2, oblique=True)
        c = core.Core(scene.scenery(geoms, 3, device='cuda', random=np.random.RandomState(3)), res=64, fov=130, fps=10)
        util.spawn(c, geoms, seed=4)
        c.agents.positions[0, 1] = c.agents.positions[0, 0] + torch.tensor([.25, .1], device='cuda')       # (two agents side by side)
        _WORLD['crowd'] = c
    return _WORLD['crowd']


def _moved(c, seed):
    """A physics step, then a render: the scenery's agent rows are the ones ms_render draws at the new poses."""
    from megastep_amd import cuda
    util.random_velocities(c, np.random.RandomState(seed))
    cuda.physics(c.scenery, c.agents)
    cuda.render(c.scenery, c.agents, fields=('distances',))


@pytest.mark.parametrize('R', [.3, 2.])
@pytest.mark.parametrize('cell,clearance', [(CELL, RADIUS), CELLS[1]])
def test_clearance_fields_are_the_rules_bits(cell, clearance, R):
    from megastep_amd import _lib, cuda
    w = _world()
    sc = w['scenery']
    grid = cuda.nav_grid(sc, cell, clearance=clearance)
    radii = (clearance, .2, .3)
    clear = cuda.clearance_fields(grid, sc, R, nearest=True, radii=radii)
    assert isinstance(clear, cuda.ClearanceFields) and clear.values.dtype == torch.float32 and clear.nearest.dtype == torch.int32
    assert clear.fits.dtype == torch.uint8 and clear.fits.shape[0] == 3*grid.n_cells and clear.radii == tuple(float(r) for r in radii)
    want = _field_rule(clear, w['rows'], _af(sc))
    same(_field(clear), want)
    finite = np.isfinite(want['values'])
    assert 0 < finite.sum() and (R > 1 or (~finite).sum() > 0)
    s, ny, nx = grid.cells(2)
    assert clear.image(2).shape == clear.nearest_image(2).shape == clear.fits_image(2, 1).shape == (ny, nx)
    assert torch.equal(clear.fits_image(2, 1).reshape(-1), clear.fits[3*s + ny*nx:3*s + 2*ny*nx].bool())
    # the other instantiation and no cull at all: the same bits
    h = _lib.lib()
    try:
        for mode in (0, 1, 2):
            h.ms_debug_nav_clear_cull(mode)
            other = cuda.clearance_fields(grid, sc, R, nearest=True, radii=radii)
            same(_field(other), want)
    finally:
        h.ms_debug_nav_clear_cull(-1)
    # values alone
    bare = cuda.clearance_fields(grid, sc, R)
    assert bare.nearest is None and bare.fits is None and torch.equal(bare.values.view(torch.int32), clear.values.view(torch.int32))


def test_fits_are_the_existing_grids_free_bytes():
    from megastep_amd import cuda
    sc = _world()['scenery']
    grid = cuda.nav_grid(sc, clearance=RADIUS)
    radii = (RADIUS, .2, .3)
    clear = cuda.clearance_fields(grid, sc, 2., radii=radii)
    for k, r in enumerate(radii):
        old = cuda.nav_grid(sc, clearance=r)
        sub = clear.nav_grid(k)
        assert sub.clearance == float(r) and sub.cell == grid.cell and sub.geom is grid.geom
        assert torch.equal(sub.free, old.free), r
        for e in range(grid.n_envs):
            assert torch.equal(clear.fits_image(e, k), old.image(e)), (r, e)
    assert torch.equal(clear.nav_grid(0).free, grid.free)
    with pytest.raises(RuntimeError, match='1.4'):
        cuda.clearance_fields(grid, sc, 2., radii=(.05,)).nav_grid(0)


def test_the_lds_list_at_and_beyond_its_boundary():
    """Every wall lies within R = 4 of every tile, so each tile keeps them all: 1100 rows run over the list (1024) and are folded and
    emptied on the way; 1024 - 256 + 1 = 769 rows are the fewest that trigger the fold before the last window."""
    from megastep_amd import _lib, cuda
    chunk = _lib.lib().ms_host_nav_clear_chunk()
    rng = np.random.RandomState(6)
    envs = []
    for count in (1100, chunk - 256 + 1, chunk - 256):
        a = rng.uniform(1., 3.5, (count//2, 2))
        short = np.stack([a, a + rng.normal(size=a.shape)*.1], 1)
        envs.append(np.concatenate([short, short[::-1], short[:count - 2*(count//2)]]))      # duplicated short walls
    c = util.custom_world(envs, 1, 64, 130, [[[2., 2.]]]*3, [[0.]]*3)
    sc = c.scenery
    grid = cuda.nav_grid(sc, clearance=RADIUS)
    clear = cuda.clearance_fields(grid, sc, 4., nearest=True, radii=(RADIUS, .5))
    rows = _rows(sc)
    assert [len(r) - _af(sc) for r in rows] == [1100, chunk - 255, chunk - 256] and grid._max_cells > 256
    want = _field_rule(clear, rows, _af(sc))
    same(_field(clear), want)
    assert (want['nearest'][:grid.n_cells] >= _af(sc)).all()            # (every cell has a winner, and never a later duplicate)
    assert (want['nearest'][:grid.cells(1)[0]] < _af(sc) + 550).all()


def test_a_masked_update_leaves_the_other_envs_alone():
    from megastep_amd import cuda, scene
    np.random.seed(5)
    sc = scene.scenery(plans(3), 1, device='cuda', random=np.random.RandomState(5), bake=False)
    grid = cuda.nav_grid(sc, clearance=RADIUS)
    clear = cuda.clearance_fields(grid, sc, 1., nearest=True, radii=(RADIUS,))
    before = _field(clear)
    sc.lines.vals.add_(.0625)                                           # every wall of every env, in place
    torch.cuda.synchronize()
    mask = torch.tensor([True, False, True], device='cuda')
    assert clear.update(mask) is clear
    after, want = _field(clear), _field_rule(clear, _rows(sc), _af(sc))
    for n in range(3):
        s, ny, nx = grid.cells(n)
        ref = want if mask[n] else before
        for key, stores in (('values', 1), ('nearest', 1), ('fits', 1)):
            a, b = after[key][stores*s:stores*(s + ny*nx)], ref[key][stores*s:stores*(s + ny*nx)]
            assert np.array_equal(a.view(np.uint32) if a.dtype == F else a, b.view(np.uint32) if b.dtype == F else b), (n, key)
    assert not np.array_equal(bits(after['values']), bits(before['values']))
    # out=: the earlier result takes this call's arguments and is written in place
    again = cuda.clearance_fields(grid, sc, 2., nearest=True, radii=(.2,), out=clear)
    assert again is clear and clear.max_range == 2. and clear.radii == (.2,)
    same(_field(clear), _field_rule(clear, _rows(sc), _af(sc)))
    with pytest.raises(RuntimeError, match='out'):
        cuda.clearance_fields(grid, sc, 2., out=clear)
    with pytest.raises(RuntimeError, match='mask'):
        clear.update(torch.ones((3, 1), dtype=torch.bool, device='cuda'))


def test_the_query_is_the_rule_at_centres_and_anywhere():
    from megastep_amd import cuda
    w = _world()
    sc, rows = w['scenery'], w['rows']
    grid = cuda.nav_grid(sc, clearance=RADIUS)
    rng = np.random.RandomState(8)
    P = 700
    points = np.zeros((3, P, 2), F)
    cells = []
    for n in range(3):
        geom = tuple(int(v) for v in grid._host_geom[n])
        x, y = nav_rule.centres(geom, CELL)
        pick = rng.randint(0, geom[2]*geom[3], 300)
        cells.append(pick)
        walls = rows[n][_af(sc):]
        lo, hi = walls.reshape(-1, 2).min(0) - 1., walls.reshape(-1, 2).max(0) + 1.
        points[n] = (lo + rng.uniform(0, 1, (P, 2))*(hi - lo)).astype(F)
        points[n, :300] = np.stack([x[pick % geom[2]], y[pick // geom[2]]], 1)
        points[n, 300] = [np.nan, 2.]
        points[n, 301] = walls[5, :2]                                   # (a wall's end: d == 0)
    pts = torch.as_tensor(points, device='cuda')
    for R in (.3, 2.):
        got = cuda.clearance(sc, pts, R)
        assert isinstance(got, cuda.Clearance) and got.distances.shape == (3, P) and got.towards.shape == (3, P, 2) and got.nearest.dtype == torch.int32
        want = query_rule(points, rows, R, sc.n_agents, sc.model.shape[0])
        same({k: _np(getattr(got, k)) for k in QUERY}, want, QUERY)
        assert (want['nearest'][:, 300] == -1).all() and (want['distances'][:, 301] == 0).all() and (want['towards'][:, 301] == 0).all()
        clear = cuda.clearance_fields(grid, sc, R, nearest=True)
        for n in range(3):
            at = torch.as_tensor(grid.cells(n)[0] + cells[n], device='cuda')
            assert torch.equal(got.distances[n, :300].view(torch.int32), clear.values[at].view(torch.int32))
            assert torch.equal(got.nearest[n, :300], clear.nearest[at])
    # a masked point keeps what out held
    out = cuda.clearance(sc, pts, 2.)
    mask = torch.as_tensor(rng.rand(3, P) < .5, device='cuda')
    full = {k: getattr(out, k).clone() for k in QUERY}
    assert cuda.clearance(sc, pts, .3, mask=mask, out=out) is out
    small = cuda.clearance(sc, pts, .3)
    for k in QUERY:
        m = mask[..., None] if k == 'towards' else mask
        assert torch.equal(getattr(out, k).view(torch.int32), torch.where(m, getattr(small, k), full[k]).view(torch.int32)), k
    with pytest.raises(RuntimeError, match='out'):
        cuda.clearance(sc, pts[:, :5].contiguous(), 2., out=out)


def test_the_query_meets_the_agents_live_rows():
    from megastep_amd import cuda
    c = _crowd()
    sc = c.scenery
    A, M = sc.n_agents, sc.model.shape[0]
    own = torch.arange(A, dtype=torch.int32, device='cuda').expand(2, A).contiguous()
    for step in range(2):
        _moved(c, 30 + step)
        rows = _rows(sc)                                                # (the render left the agents' drawn rows in the scenery)
        here = c.agents.positions.clone()
        points = _np(here)
        for skip in (own, torch.full_like(own, -1), torch.tensor([[2, 9, 0], [-3, 1, 1]], dtype=torch.int64, device='cuda'), None):
            got = cuda.clearance(sc, here, 2., agents=c.agents, skip=skip)
            want = query_rule(points, rows, 2., A, M, True, None if skip is None else _np(skip))
            same({k: _np(getattr(got, k)) for k in QUERY}, want, QUERY)
            if skip is own:
                assert (want['nearest']//M != _np(own)).all()           # (nobody's nearest is its own body)
        static = cuda.clearance(sc, here, 2.)
        same({k: _np(getattr(static, k)) for k in QUERY}, query_rule(points, rows, 2., A, M, False), QUERY)
        assert ((_np(static.nearest) >= A*M) | (_np(static.nearest) < 0)).all()


def test_proximity_replays_as_it_runs_eagerly():
    from megastep_amd import cuda, modules
    c = _crowd()
    prox = modules.Proximity(c, max_range=1.5)
    assert prox.space.shape == modules.spaces.MultiVector(c.n_agents, 3).shape
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        prox()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        obs = prox()
    for step in range(3):
        _moved(c, 40 + step)
        g.replay()
        eager = modules.Proximity(c, max_range=1.5)()
        assert obs.shape == (c.n_envs, c.n_agents, 3) and torch.equal(obs.view(torch.int32), eager.view(torch.int32))
        reading = cuda.clearance(c.scenery, c.agents.positions, 1.5, agents=c.agents, skip=prox._skip)
        assert torch.equal(obs[..., 0], (reading.distances/1.5).clamp(max=1.))
        assert torch.equal(obs[..., 1:], modules.to_local_frame(c.agents.angles, reading.towards))
    # without the others the reading is the static query's
    alone = modules.Proximity(c, max_range=1.5, others=False)()
    static = cuda.clearance(c.scenery, c.agents.positions, 1.5)
    assert torch.equal(alone.view(torch.int32), modules.Proximity.observation(static.distances, static.towards, c.agents.angles, 1.5).view(torch.int32))
    assert (alone[..., 0] >= obs[..., 0]).all()                         # (fewer lines to be near to)


def test_the_layer_feeds_draws_windows_and_regions():
    from megastep_amd import cuda
    w = _world()
    sc = w['scenery']
    grid = cuda.nav_grid(sc, clearance=RADIUS)
    R = 2.
    radii = (RADIUS, .2, .3)
    clear = cuda.clearance_fields(grid, sc, R, radii=radii)
    # spawns half a metre from any wall
    draws = cuda.cell_draws(grid, clear, 1, 64, lo=.5, hi=float('inf'))
    values, free = _np(clear.values), _np(grid.free)
    for n in range(3):
        s, ny, nx = grid.cells(n)
        count = int(((values[s:s + ny*nx] >= F(.5)) & (free[s:s + ny*nx] != 0)).sum())
        assert int(draws.counts[n, 0]) == count > 0
        cells = _np(draws.cells[n, 0])
        assert (cells >= 0).all() and (values[s + cells] >= F(.5)).all() and np.array_equal(bits(_np(draws.values[n, 0])), bits(values[s + cells]))
    # a distance-to-obstacle channel of the policy's map
    views = cuda.plan_views(sc, 24)
    window_same(grid, views, 24, [cuda.map_channel(clear, scale=1/R)])
    # the floor a larger body can reach is no larger
    regions = cuda.regions(grid, marks=clear.fits, n_fields=3)
    open_cells = _np(regions.open_cells)
    assert (open_cells[:, 0] >= open_cells[:, 1]).all() and (open_cells[:, 1] >= open_cells[:, 2]).all() and (open_cells[:, 2] > 0).all()
    assert np.array_equal(open_cells[:, 0], _np(cuda.regions(grid).open_cells)[:, 0])
