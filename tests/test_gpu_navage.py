"""Age maps on the GPU: `AgeMaps.mark` equal to the numpy statement of the contract (tests/test_navage_host.age_rule) - the ticks,
the clocks, swept, gained, idle and every output of the survey, exactly - on the distances of real `cuda.render` frames, with a
map per agent and with one shared by an env's agents; hand-made grids at the bitmask's word edges and of more than 64 KiB of bits, an env without cells, skipped
viewers, NaN inputs and the clock at its cap; a large plan; the survey alone and the marks alone; `out=`, streams and graph
capture; the maps as layers of the other nav calls; and the `Patrol` env, eager and as one HIP graph."""
import numpy as np
import pytest
import torch

from tests.test_navfield_host import CELL, RADIUS, F, plans
from tests.test_navage_host import CAP, COUNTS, SURVEY, age_rule
from tests.test_gpu_navseen import _actions, _by_hand, _core, _fans, _frame, _np
from tests.test_gpu_navseen import _odd_calls as _wide_calls, _odd_grid as _wide_grid

pytestmark = pytest.mark.gpu


class _Mirror:
    """age_rule's copy of an AgeMaps: the ticks and clocks of every env, moved on call by call."""

    def __init__(self, ages, cell=CELL):
        grid = ages.grid
        self.cell, self.S, self.threshold = cell, ages.n_maps, ages.threshold
        self.geom = [tuple(int(v) for v in g) for g in _np(grid.geom)]
        self.spans = [(grid.cells(e)[0], grid.cells(e)[1]*grid.cells(e)[2]) for e in range(grid.n_envs)]
        self.countable = [_np(ages.countable)[at:at + n] for at, n in self.spans]
        self.last = [_np(ages.last)[self.S*at:self.S*(at + n)].reshape(self.S, g[3], g[2]).copy() for (at, n), g in zip(self.spans, self.geom)]
        self.clock = _np(ages.clock).copy()
        self.found = None

    def call(self, origins=None, dirs=None, distances=None, slot=None, max_range=10., reset=None, advance=True, survey=True):
        origins, dirs, distances, slot, reset = (_np(t) for t in (origins, dirs, distances, slot, reset))
        each = lambda t, e: None if t is None else t[e]
        found = []
        for e, geom in enumerate(self.geom):
            got = age_rule.call(geom, self.cell, self.countable[e], self.last[e], self.clock[e], each(origins, e), each(dirs, e), each(distances, e),
                                slot=each(slot, e), max_range=max_range, reset=each(reset, e), advance=advance, threshold=self.threshold, survey=survey)
            self.last[e], self.clock[e] = got['last'], got['clock']
            found.append(got)
        if survey:
            self.found = found
        return found

    def check(self, ages, sweep, found):
        """The maps, the clocks and the sweep against the call's numbers; the survey's outputs against the last survey's."""
        assert np.array_equal(_np(ages.clock), self.clock), (_np(ages.clock), self.clock)
        if sweep is not None:
            for k in COUNTS:
                got, want = _np(getattr(sweep, k)), np.stack([f[k] for f in found])
                assert got.dtype == want.dtype and np.array_equal(got, want), (k, got, want)
        for e in range(len(self.geom)):
            for s in range(self.S):
                got = _np(ages.image(e, s))
                assert np.array_equal(got, self.last[e][s]), (e, s, int((got != self.last[e][s]).sum()))
        if self.found is not None:
            for k in ('oldest', 'total_age', 'n_stale'):
                got, want = _np(getattr(ages, k)), np.stack([f[k] for f in self.found])
                assert got.dtype == want.dtype and np.array_equal(got, want), (k, got, want)
            for e in range(len(self.geom)):
                for s in range(self.S):
                    assert np.array_equal(_np(ages.age_image(e, s)), self.found[e]['ages'][s]), (e, s)
                    assert np.array_equal(_np(ages.stale_image(e, s)), self.found[e]['stale'][s].astype(bool)), (e, s)


_SIX = {}


def _six():
    """The six plans (three plain, three oblique), two agents each, 64 rays, and four frames of them with the agents turned and
    moved in between - shared by the tests."""
    if not _SIX:
        geoms = plans(3) + plans(3, oblique=True)
        c = _core(geoms, 2, 64)
        frames = [_frame(c)]
        for turn, move in ((100., (.3, .2)), (-40., (-.2, .25)), (170., (.1, -.3))):
            c.agents.angles[:] = c.agents.angles + turn
            c.agents.positions[:] = c.agents.positions + torch.tensor(move, device='cuda')
            frames.append(_frame(c))
        _SIX.update(core=c, geoms=geoms, frames=frames)
    return _SIX


def _grid():
    from megastep_amd import cuda
    return cuda.nav_grid(_six()['core'].scenery, clearance=RADIUS)


@pytest.mark.parametrize('shared', [False, True])
def test_mark_is_the_rule_on_rendered_frames(shared):
    from megastep_amd import cuda
    w = _six()
    ages = cuda.age_maps(_grid(), 1 if shared else 2, threshold=2)
    mirror = _Mirror(ages)
    slot = torch.zeros((6, 2), dtype=torch.int64, device='cuda') if shared else None
    rng = np.random.RandomState(4)
    swept = idle = 0
    for k, frame in enumerate(w['frames']):
        reset = torch.as_tensor(rng.rand(6, ages.n_maps) < .5, device='cuda') if k == 2 else None
        assert reset is None or (reset.any() and not reset.all())
        sweep = ages.mark(*frame, slot=slot, reset=reset)
        found = mirror.call(*frame, slot=slot, reset=reset)
        mirror.check(ages, sweep, found)
        swept, idle = swept + int(sweep.swept.sum()), idle + int(sweep.idle.sum())
        assert (sweep.gained <= sweep.swept).all()
    assert swept > 3000 and idle > swept and int(ages.n_stale.sum()) > 0 and 1 <= int(ages.clock.min()) < int(ages.clock.max()) == 4
    assert np.array_equal(_np(ages.mean_age()), _np(ages.total_age).astype(F)/np.maximum(_np(ages.n_countable), 1)[:, None].astype(F))


ODD_SHAPES = [(31, 1), (0, 0), (32, 1), (33, 1), (9, 7), (8, 8), (13, 5), (1, 40), (40, 1), (1, 1), (0, 3), (56, 40)]


def _odd_maps(device='cuda'):
    """Maps over envs at the bitmask's word edges, one without cells between two with, one row, one column, one cell; some
    clocks a tick from the cap and at it."""
    from megastep_amd import cuda
    rng = np.random.RandomState(12)
    grid = _by_hand([((-3 + k, 2 - k, nx, ny), rng.rand(ny, nx) < .8) for k, (nx, ny) in enumerate(ODD_SHAPES)], device)
    ages = cuda.age_maps(grid, 2, threshold=3)
    ages.clock[::2, 0] = CAP - 1                                         # (the next tick is the last)
    ages.clock[3] = CAP
    ages.last[:31] = float(CAP - 5)                                      # (map (0, 0), whole)
    return ages


def _odd_calls(grid, device='cuda'):
    """Four calls' keywords: three viewers an env inside its first cell, its last and between, slots that skip some, resets, and
    in the third NaN, infinite and negative inputs."""
    rng = np.random.RandomState(9)
    n = grid.n_envs
    geom = _np(grid.geom)
    lo = (geom[:, :2] + .5)*CELL
    hi = (geom[:, :2] + np.maximum(geom[:, 2:], 1) - .5)*CELL
    centres = np.stack([lo, hi, (lo + hi)/2], 1)
    for trial in range(4):
        origins, dirs, distances = _fans(rng, centres + rng.uniform(-.04, .04, centres.shape), 11, 3., device)
        slot = torch.as_tensor(rng.randint(-1, 3, (n, 3)), device=device)                  # (-1 and 2: nobody's map)
        reset = torch.as_tensor(rng.rand(n, 2) < .3, device=device) if trial else None
        if trial == 2:
            distances[:, :, ::5] = float('nan'); distances[:, :, 1::7] = float('inf'); distances[:, 0, 2] = 0.; distances[:, 1, 3] = -2.
            dirs[:, 1, 4] = float('nan'); dirs[:, 2, 6, 1] = float('inf'); dirs[:, 0, 8] = 0.
            origins[2, 1, 0] = float('nan'); origins[0, 2] = float('-inf')
        yield dict(origins=origins, dirs=dirs, distances=distances, slot=slot, reset=reset, max_range=2.)


def test_word_edges_an_env_without_cells_skipped_viewers_nans_and_the_clock_at_its_cap():
    assert sorted(nx*ny for nx, ny in ODD_SHAPES)[2:11] == [1, 31, 32, 33, 40, 40, 63, 64, 65]
    ages = _odd_maps()
    mirror = _Mirror(ages)
    marked = 0
    for call in _odd_calls(ages.grid):
        sweep = ages.mark(**call)
        found = mirror.call(**call)
        mirror.check(ages, sweep, found)
        assert found[1]['swept'].tolist() == found[10]['swept'].tolist() == [0, 0]
        marked += sum(int(f['swept'].sum()) for f in found)
    assert marked > 500 and int(ages.clock.max()) == CAP and int(ages.oldest.max()) > 2**23


def test_a_grid_of_more_than_64_kib_of_bits():
    """The seen suite's hand-made grid, whose last env has 640 800 cells: 80 100 bytes of bitmask, beyond the 64 KiB a launch gets
    without asking - with its calls' resets, skipped viewers and NaN inputs."""
    from megastep_amd import cuda
    grid = _wide_grid()
    assert (grid._max_cells + 31)//32*4 > 64*1024
    ages = cuda.age_maps(grid, 2, threshold=2)
    mirror = _Mirror(ages)
    for origins, dirs, distances, slot, reset, max_range in _wide_calls():
        sweep = ages.mark(origins, dirs, distances, slot=slot, reset=reset, max_range=max_range)
        found = mirror.call(origins, dirs, distances, slot=slot, reset=reset, max_range=max_range)
        mirror.check(ages, sweep, found)
        assert found[1]['swept'].tolist() == [0, 0] and found[3]['swept'].sum() > 0
    assert int(ages.total_age[3].min()) > 600000                         # (the large env's cells, nearly all a tick old or more)


def test_a_large_plan_with_many_words_a_lane_and_rays_cut_by_max_range():
    from megastep_amd import cuda
    c = _core(plans(1, large=True), 2, 256, seed=3)
    grid = cuda.nav_grid(c.scenery, clearance=RADIUS)
    assert grid.n_cells > 32*256*4                                       # (more than four words of the bitmask per lane)
    ages = cuda.age_maps(grid, 2, threshold=2)
    mirror = _Mirror(ages)
    frame = _frame(c)
    assert (frame[2] > 1.5).float().mean() > .5                          # (most rays are cut at 1.5 m)
    for max_range in (10., 1.5, 10.):
        sweep = ages.mark(*frame, max_range=max_range)
        mirror.check(ages, sweep, mirror.call(*frame, max_range=max_range))
    assert (_np(sweep.swept) > 0).all() and int(sweep.idle.sum()) > int(sweep.swept.sum()) and int(ages.n_stale.sum()) > 300


def test_the_survey_alone_and_the_marks_alone():
    from megastep_amd import cuda
    w = _six()
    ages = cuda.age_maps(_grid(), 2, threshold=2)
    mirror = _Mirror(ages)
    first = ages.mark(*w['frames'][0])
    mirror.check(ages, first, mirror.call(*w['frames'][0]))
    kept = {k: getattr(ages, k).clone() for k in SURVEY}
    for frame in w['frames'][1:3]:                                       # the marks alone: the survey's outputs stand
        sweep = ages.mark(*frame, survey=False)
        found = mirror.call(*frame, survey=False)
        mirror.check(ages, sweep, found)
        assert all(torch.equal(getattr(ages, k), kept[k]) for k in SURVEY)
    before = (ages.last.clone(), ages.clock.clone())
    assert ages.survey() is ages                                         # the survey alone: the maps and the clocks stand
    mirror.call(advance=False)
    mirror.check(ages, None, None)
    assert torch.equal(ages.last, before[0]) and torch.equal(ages.clock, before[1]) and int(ages.clock.max()) == 3
    assert not torch.equal(ages.ages, kept['ages']) and int(ages.oldest.max()) == 3 and int(ages.n_stale.min()) > 0
    bare = cuda.age_maps(_grid(), 2, threshold=2, ages=False)            # ... and without the store of ages
    bare.mark(*w['frames'][0])
    full = cuda.age_maps(_grid(), 2, threshold=2)
    full.mark(*w['frames'][0])
    assert bare.ages is None and torch.equal(bare.stale, full.stale) and torch.equal(bare.total_age, full.total_age) and torch.equal(bare.last, full.last)


def test_out_a_side_stream_and_a_graph_replayed_three_times():
    from megastep_amd import cuda
    w = _six()
    grid = _grid()
    origins, dirs, distances = (t.clone() for t in w['frames'][0])
    ages = cuda.age_maps(grid, 2, threshold=2)
    mirror = _Mirror(ages)
    out = cuda.Sweep(*(torch.full((6, 2), -5, dtype=d, device='cuda') for d in (torch.int32, torch.int32, torch.int64)))
    assert ages.mark(origins, dirs, distances, out=out) is out
    mirror.check(ages, out, mirror.call(origins, dirs, distances))
    with pytest.raises(RuntimeError, match='out'):
        ages.mark(origins, dirs, distances, out=torch.zeros((6, 2), dtype=torch.int32, device='cuda'))
    with pytest.raises(RuntimeError, match='out'):
        ages.mark(origins, dirs, distances, out=cuda.Sweep(out.swept, out.gained, out.swept))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        there = ages.mark(*w['frames'][1], max_range=3.)
    side.synchronize()
    mirror.check(ages, there, mirror.call(*w['frames'][1], max_range=3.))
    # a graph of one mark replayed three times is three eager calls: ticks 1, 2, 3 of fresh maps, the clock on the device
    graphed, eager = cuda.age_maps(grid, 2, threshold=2), cuda.age_maps(grid, 2, threshold=2)
    reset = torch.zeros((6, 2), dtype=torch.bool, device='cuda')
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        cuda.age_maps(grid, 2).mark(origins, dirs, distances, reset=reset, out=cuda.Sweep(*(torch.empty_like(t) for t in (out.swept, out.gained, out.idle))))
    torch.cuda.current_stream().wait_stream(side)
    with torch.cuda.graph(graph):
        sweep = graphed.mark(origins, dirs, distances, reset=reset, out=out)
    assert int(graphed.clock.max()) == 0                                 # (captured, not run)
    mirror = _Mirror(graphed)
    rng = np.random.RandomState(2)
    for trial in range(3):
        frame = w['frames'][trial + 1]
        origins.copy_(frame[0] + torch.as_tensor(rng.uniform(-.1, .1, (6, 2, 2)).astype(F), device='cuda'))
        dirs.copy_(frame[1]); distances.copy_(frame[2])
        reset.copy_(torch.as_tensor(rng.rand(6, 2) < .2, device='cuda') if trial == 2 else torch.zeros_like(reset))
        graph.replay()
        want = eager.mark(origins, dirs, distances, reset=reset)
        assert all(torch.equal(getattr(sweep, k), getattr(want, k)) for k in COUNTS)
        assert torch.equal(graphed.last, eager.last) and torch.equal(graphed.clock, eager.clock)
        assert all(torch.equal(getattr(graphed, k), getattr(eager, k)) for k in SURVEY)
        mirror.check(graphed, sweep, mirror.call(origins, dirs, distances, reset=reset))
        assert int(graphed.clock.max()) == trial + 1
    assert int(graphed.clock.min()) == 1 and int(sweep.idle.sum()) > 0


def _marked(w, shared, threshold):
    from megastep_amd import cuda
    ages = cuda.age_maps(_grid(), 1 if shared else 2, threshold=threshold)
    slot = torch.zeros((6, 2), dtype=torch.int64, device='cuda') if shared else None
    mirror = _Mirror(ages)
    for frame in w['frames']:
        ages.mark(*frame, slot=slot, max_range=3.)
        mirror.call(*frame, slot=slot, max_range=3.)
    return ages, slot, mirror


@pytest.mark.parametrize('shared', [False, True])
def test_the_maps_are_layers_of_the_other_nav_calls(shared):
    from megastep_amd import cuda
    from tests.test_gpu_navwindow import _same as window_same
    w = _six()
    T = 2
    ages, slot, mirror = _marked(w, shared, T)
    grid, S = ages.grid, ages.n_maps
    # stale_fields: seeded_fields on the marks numpy makes of the rule's ticks
    marks = torch.zeros_like(ages.stale)
    for e, (at, n) in enumerate(mirror.spans):
        old = (mirror.clock[e][:, None, None] - mirror.last[e].astype(np.int64) >= T) & (mirror.countable[e].reshape(mirror.last[e].shape[1:]) & 1).astype(bool)
        marks[S*at:S*(at + n)] = torch.as_tensor(old.astype(np.uint8).reshape(-1), device='cuda')
    assert 0 < int(marks.sum()) < int(ages.n_countable.sum())*S
    fields, want = ages.stale_fields(), cuda.seeded_fields(grid, marks, S)
    assert fields.marks.data_ptr() == ages.stale.data_ptr()              # (read by reference)
    assert torch.equal(fields.values.view(torch.int32), want.values.view(torch.int32)) and torch.equal(fields.n_seeds, want.n_seeds)
    assert torch.isfinite(fields.values).any() and int(fields.n_seeds.min()) > 0
    assert torch.equal(ages.stale_regions().labels, cuda.regions(grid, marks, S).labels)
    priced = ages.stale_fields(cost=cuda.mark_costs(ages, on=1., off=3.))
    assert isinstance(priced, cuda.CostFields) and torch.equal(priced.n_seeds, want.n_seeds)
    # cell_draws in the band [T, inf): only cells whose age is at least T
    draws = cuda.cell_draws(grid, ages, S, 8, lo=T, hi=float('inf'))
    cells, counts, values = _np(draws.cells), _np(draws.counts), _np(draws.values)
    assert (cells >= 0).all()
    for e in range(6):
        free = _np(grid.image(e)).astype(bool)
        for s in range(S):
            age = mirror.found[e]['ages'][s]
            assert counts[e, s] == int(((age >= T) & free).sum())
            assert (age.reshape(-1)[cells[e, s]] >= T).all() and free.reshape(-1)[cells[e, s]].all()
            assert np.array_equal(values[e, s], age.reshape(-1)[cells[e, s]])
    # local_maps with the ages over T as a channel, and the stale cells as a gate
    c = w['core']
    age = cuda.cell_layer(ages, field=slot)
    channels = [cuda.map_channel(age, scale=1/T), cuda.map_channel(grid, gate=cuda.cell_layer(ages.stale, S, field=slot))]
    got = _np(window_same(grid, cuda.agent_views(c.agents, 24, 3.), 24, channels))
    assert ((got[:, :, 0] > 0) & (got[:, :, 0] < 1)).any() and (got[:, :, 0] == 1).any() and (got[:, :, 0] == 0).any() and got[:, :, 1].sum() > 0
    if not shared:
        gated = cuda.local_maps(grid, cuda.agent_views(c.agents, 24, 3.), 24, [cuda.map_channel(grid, gate=ages)])
        assert np.array_equal(_np(gated)[:, :, 0], got[:, :, 1])         # (as a gate the maps present their stale cells)


def test_idleness_and_patrols_are_the_calls_they_stand_for():
    from megastep_amd import cuda, modules
    w = _six()
    c, grid = w['core'], _grid()
    for shared in (False, True):
        idle = modules.Idleness(c, grid, max_range=4., shared=shared, threshold=2)
        plain = cuda.age_maps(grid, 1 if shared else 2, threshold=2)
        slot = torch.zeros((6, 2), dtype=torch.int64, device='cuda') if shared else None
        for k in range(3):
            c.agents.angles[:] = c.agents.angles + 50.
            frame = modules.render(c, fields=('distances',))
            reset = torch.zeros((6, 2), dtype=torch.bool, device='cuda')
            reset[1, 0] = k == 2
            reward = idle(frame, reset)
            want = plain.mark_render(c.agents, frame, slot=slot, max_range=4., reset=reset.any(-1, keepdim=True) if shared else reset)
            expected = (want.idle - want.swept).float()*F(CELL)**2/2
            assert reward.shape == (6, 2) and torch.equal(reward, expected.expand(-1, 2) if shared else expected)
            assert torch.equal(idle.ages.last, plain.last) and torch.equal(idle.ages.clock, plain.clock)
        assert (reward >= 0).all() and reward.sum() > 0 and int(idle.ages.clock[1, 0]) == 1 and int(idle.ages.clock[2, 0]) == 3
        obs = idle.observation()
        assert obs.shape == (6, 2, 2) and idle.space.shape == (2, 2) and (obs >= 0).all() and (obs <= 1).all()
        per = lambda t: t.expand(-1, 2) if shared else t
        assert torch.equal(obs[..., 0], per((plain.mean_age()/2).clamp(max=1.))) and torch.equal(obs[..., 1], per((plain.oldest.float()/2).clamp(max=1.)))
        assert idle.state(2).shape == (plain.n_maps,) + tuple(plain.image(2).shape)
        patrols = modules.Patrols(c, idle, refresh=2)
        fields = patrols(reset)
        assert patrols.due.all() and torch.equal(fields.values.view(torch.int32), plain.stale_fields().values.view(torch.int32))
        way, far = patrols.waypoints(), patrols.distance()
        assert way.shape == (6, 2, 2) and far.shape == (6, 2) and (torch.isnan(way).any(-1) | ~torch.isinf(far)).all()
        assert torch.isfinite(far).any()
        patrols()
        assert not patrols.due.any()
        action = modules.PathFollower(c, patrols)().actions
        assert action.shape == (6, 2) and ((action >= 0) & (action < 7)).all()


def test_patrol_as_a_hip_graph_equals_the_eager_env_and_the_expert_acts():
    from megastep_amd import arrdict, graphs
    from megastep_amd.demo import Patrol
    rng = np.random.RandomState(8)
    acts = [_actions(rng, 8, 2) for _ in range(12)]
    logs = []
    for graphed in (False, True):
        torch.manual_seed(3); np.random.seed(3)
        env = Patrol(8, 2, geometries=plans(8), threshold=4, local_map=True, max_lifespan=10**6)
        stepper = graphs.GraphedStep(env, warmup=3) if graphed else env
        world = stepper.reset()
        assert world.reset.all() and world.obs.idleness.shape == (8, 2, 2) and world.obs['map'].shape == (8, 2, 3, 32, 32)
        log = []
        # the graphed env's first step call is four steps under its actions: three of warm-up and the captured one
        for a in (acts if graphed else [acts[0]]*3 + acts):
            world = stepper.step(arrdict.arrdict(actions=a))
            log.append((world.reward.clone(), world.reset.clone(), world.obs.idleness.clone(), world.obs['map'].clone(), world.obs.rgb.clone(),
                        world.obs.d.clone(), env.ages.last.clone(), env.ages.clock.clone()))
        logs.append(log)
    eager, graphed = logs
    for k in range(12):
        for got, want in zip(graphed[k], eager[k + 3]):
            assert torch.equal(got, want), k
    assert sum(float(log[0].sum()) for log in graphed) > 0 and int(graphed[-1][7].min()) == 16 and graphed[-1][3][:, :, 2].max() == 1
    assert env.obs_space.idleness.shape == (2, 2) and env.obs_space['map'].shape == (2, 3, 32, 32)
    actions = env.expert().actions
    assert actions.shape == (8, 2) and actions.dtype == torch.int64 and ((actions >= 0) & (actions < 7)).all()
    assert (actions > 0).any() and env.state(0).ages.shape[0] == 1
    # episodes end by lifespan only, and an agent that starts over clears the env's map and its clock
    torch.manual_seed(5); np.random.seed(5)
    env = Patrol(8, 2, geometries=plans(8), threshold=4, max_lifespan=8)
    env.reset()
    starts = 0
    for t in range(12):
        world = env.step(env.expert())
        clock = _np(env.ages.clock)[:, 0]
        assert np.array_equal(clock == 1, _np(world.reset))
        starts += int(world.reset.sum())
    assert 0 < starts < 8*12
