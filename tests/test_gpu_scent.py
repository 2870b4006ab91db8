"""nav_scent_kernel and nav_scent_query_kernel through cuda.scent_fields against tests/scent_rule.py, AS BITS: the host suite's
cases on the device, every LDS tier's edge, the global path, the source counts, and the calls in streams and graphs."""
import types
import numpy as np
import pytest
import torch
from tests.scent_rule import F
from tests.test_scent_host import ORDERS, hand_world, mixed_ticks, ordered, sniff, subnormals, tick, world

pytestmark = pytest.mark.gpu
_t = lambda a, dtype=None: None if a is None else torch.as_tensor(np.asarray(a, dtype), device='cuda')


def fields(w):
    """w's grid and stores on the device, made at the first call."""
    from megastep_amd import cuda
    from tests.test_gpu_navseen import _by_hand
    if not hasattr(w, 'dev'):
        w.dev = cuda.scent_fields(_by_hand(w.envs, cell=w.cell, clearance=.1 if w.cell < .14 else w.cell), w.G)
        assert (w.dev._workspace is not None) == (w.max_framed > cuda.SCENT_CAPACITY[-1])
    return w.dev


def device_tick(w, points, amounts, field, reset, mask, rate, keep, floor, T):
    s = fields(w)
    s.rate, s.keep, s.floor, s.substeps = rate, keep, floor, T
    s.step(_t(points), _t(amounts), _t(field), _t(reset, bool), _t(mask, bool))
    w.V[:], w.peaks[:], w.scented[:] = s.values.cpu().numpy(), s.peaks.cpu().numpy(), s.scented.cpu().numpy()
    return 0


def device_sniff(w, points, field, out, grads):
    got = fields(w).sniff(_t(points), _t(field))
    out[:], grads[:] = got.values.cpu().numpy(), got.gradients.cpu().numpy()
    return 0


device = types.SimpleNamespace(tick=device_tick, sniff=device_sniff)


@pytest.mark.parametrize('side', [99, 100, 141, 142, 200, 201])
def test_each_tier_at_its_largest_square_and_one_more(side):
    """(side + 2)^2 against SCENT_CAPACITY = (10224, 20464, 40944): 99, 141 and 200 are the largest squares of their tiers, one more
    is the next tier and, beyond the last, the global path with its workspace; a 9 x 7 env beside each; two stores, T = 3."""
    from tests.test_navregion_host import serpentine
    w = world([((-3, 2, side, side), serpentine(side)), ((0, 0, 9, 7), np.ones((7, 9), bool))], 2)
    rng = np.random.RandomState(side)
    for _ in range(2):
        points = (rng.rand(2, 9, 2)*np.array([[[side*.125]], [[.9]]]) + np.array([[[-.375, .25]], [[0., 0.]]])).astype(F)
        tick(w, device, points=points, amounts=rng.rand(2, 9).astype(F), field=rng.randint(0, 2, (2, 9)).astype(np.int32), T=3)
    sniff(w, device, points, rng.randint(-1, 3, (2, 9)).astype(np.int32))
    assert w.scented.min() > 3


@pytest.mark.parametrize('T', [2, 3])
def test_the_global_path_at_size_lands_in_values_at_odd_and_even_T(T):
    from tests.test_gpu_navseen import _odd_grid
    grid = _odd_grid('cpu')
    w = world([(tuple(int(v) for v in grid._host_geom[e]), grid.image(e).numpy()) for e in (3, 1)], 1)
    points = (np.random.RandomState(T).rand(2, 70, 2)*F(90.) - F(45.)).astype(F)
    tick(w, device, points=points, amounts=np.ones((2, 70), F), T=T)
    tick(w, device, T=T)
    sniff(w, device, points)
    assert w.scented[0, 0] > 70 and w.scented[1, 0] == 0


@pytest.mark.parametrize('P', [1, 64, 65, 1024])
def test_many_sources_colliding_on_few_cells(P):
    rng = np.random.RandomState(P)
    w = hand_world()
    spots = np.array([[.3, .15], [.45, .15], [.8, .7], [.45, .55], [.14, .01]], F)      # four open cells of env 0 and its closed (0, 1)
    for _ in range(2):
        amounts = (rng.choice([1., 3e-8, 2.**-24, 2.**-23, .3, 100.], (3, P))*rng.rand(3, P)).astype(F)
        tick(w, device, points=spots[rng.randint(0, 5, (3, P))], amounts=amounts, field=rng.randint(-1, 3, (3, P)).astype(np.int32), T=2)
    assert P < 64 or w.scented[:2].min() > 0


@pytest.mark.parametrize('T', [1, 64])
def test_the_hand_made_grid_with_odd_sources_resets_and_masks(T):
    mixed_ticks(hand_world(), device, T)


@pytest.mark.parametrize('resident,amounts', ORDERS)
def test_sources_on_one_cell_add_in_ascending_order(resident, amounts):
    ordered(device, resident, amounts)


def test_subnormal_values_are_not_flushed():
    subnormals(hand_world(G=1), device)


def _ticks(t):
    rng = np.random.RandomState(40 + t)
    return _t((rng.rand(3, 5, 2)*.8).astype(F)), _t(rng.rand(3, 5).astype(F)), _t(rng.randint(0, 2, (3, 5)).astype(np.int32))


def test_a_step_on_a_side_stream_and_step_and_sniff_in_a_graph_replayed_three_times():
    eager, graphed = fields(hand_world()), fields(hand_world())
    points, amounts, field = (t.clone() for t in _ticks(0))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                       # (the warm-up tick, on a side stream: both take it)
        graphed.step(points, amounts, field)
        out = graphed.sniff(points, field)
    torch.cuda.current_stream().wait_stream(side)
    eager.step(points, amounts, field)
    assert torch.equal(eager.values.view(torch.int32), graphed.values.view(torch.int32)) and eager.values.sum() > 0
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        graphed.step(points, amounts, field)
        graphed.sniff(points, field, out=out)
    for t in range(1, 4):
        for held, new in zip((points, amounts, field), _ticks(t)):
            held.copy_(new)
        graph.replay()
        want = eager.step(points, amounts, field).sniff(points, field)
        for a, b in ((eager.values, graphed.values), (eager.peaks, graphed.peaks), (want.values, out.values), (want.gradients, out.gradients)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), t
        assert torch.equal(eager.scented, graphed.scented) and out.values.sum() > 0


class _Walk:
    """Two agents an env on a walk their actions steer, leaving a scent: the least env graphs.GraphedStep takes."""

    def __init__(self, own):
        from megastep_amd import core, cuda, modules, scene, toys
        scenery = scene.scenery(3*[toys.box()], 2, device='cuda', bake=False)
        self.core = core.Core(scenery)
        self.device = self.core.device
        self.scent = modules.Scent(self.core, cuda.nav_grid(scenery, clearance=.1), amount=2., own=own, substeps=2)
        self.core.agents.positions[:] = torch.tensor([[2.5, 3.], [3.5, 3.25]], device='cuda')

    def step(self, decision):
        from megastep_amd import arrdict
        agents = self.core.agents
        agents.positions.add_((decision.actions.float() - 1.)*.07)
        agents.angles.add_(25.)
        self.scent(reset=decision.actions[:, 0, 0] == 2)
        return arrdict.arrdict(obs=self.scent.observation(), peaks=self.scent.fields.peaks)


@pytest.mark.parametrize('own', [False, True])
def test_the_scent_module_under_a_graphed_step_is_the_eager_module(own):
    from megastep_amd import arrdict, graphs
    eager, graphed = _Walk(own), graphs.GraphedStep(_Walk(own), warmup=1)
    for t in range(8):
        decision = arrdict.arrdict(actions=torch.as_tensor(np.random.RandomState(t).randint(0, 3, (3, 2, 2)), device='cuda'))
        if t == 0:
            eager.step(decision)                                        # (the graphed env's first call steps once to warm up)
        want, got = eager.step(decision), graphed.step(decision)
        assert torch.equal(want.obs.view(torch.int32), got.obs.view(torch.int32)) and torch.equal(want.peaks, got.peaks), t
        assert torch.equal(eager.scent.fields.values.view(torch.int32), graphed.scent.fields.values.view(torch.int32))
    assert want.obs.abs().sum() > 0 and eager.scent.fields.n_fields == (2 if own else 1)
