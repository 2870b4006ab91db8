"""Sliding walkers on the GPU: walker_slide_kernel - both instantiations - held to EQUALITY with its host instantiation, which the CPU
suite holds to walk_slide_rule, in the whole store and every record, floats by their bits."""
import numpy as np
import pytest
import torch

from tests import walker_rule as wr
from tests import walker_slide_rule as ws
from tests.walker_rule import NAN
from tests.test_navfield_host import RADIUS as AGENT_RADIUS, plans
from tests.test_gpu_navseen import _np
from tests.test_gpu_walkers import _dev, _world

pytestmark = pytest.mark.gpu

# the worlds' seeds, 7 A + P + 100 x: chosen on the CPU, by the host statement alone, so that every world has a walker that slides, one that
# is left at rest and one whose phase-B reach is beyond the near lists (the test asserts all three)
SEEDS = {(1, 1): 0, (1, 5): 0, (63, 1): 2, (63, 5): 2, (64, 1): 17, (64, 5): 2, (65, 1): 5, (65, 5): 5, (258, 1): 4, (258, 5): 4, (1024, 1): 2, (1024, 5): 0}


def _tick(sc, agents, walls, store, towards, dev, load=True, walk=None, slide=True, **kw):
    """One tick on the device - cuda.walk(slide=), or `walk()` - and by the host statement from the numpy `store`, compared: the store after it."""
    from megastep_amd import core, cuda
    for k in wr.STORE + ('speeds',) if load else ():
        getattr(dev, k).copy_(_dev(store[k]))
    walked = walk() if walk else cuda.walk(sc, agents, dev, towards, slide=slide, **{k: _dev(v) if isinstance(v, np.ndarray) else v for k, v in kw.items()})
    torch.cuda.synchronize()
    keys, host = (ws.KEYS, ws.host_walk_slide) if slide else (wr.KEYS, wr.host_walk)
    want = host(walls, _np(agents.positions), store, _np(towards), radius=core.AGENT_RADIUS, **(slide if isinstance(slide, dict) else {}), **kw)
    wr.same({k: _np(getattr(dev if k in wr.STORE else walked, k)) for k in keys}, want, keys)
    assert slide or (walked.slid is None and walked.stopped is None)
    return dict(store, **{k: want[k] for k in wr.STORE}), want


@pytest.mark.parametrize('N,bake', [(1, True), (5, True), (5, False)])
@pytest.mark.parametrize('A,P', [(1, 1), (5, 63), (1, 64), (5, 65), (5, 258), (1, 1024)])
def test_the_sliding_kernel_is_its_host_statement_in_both_instantiations(A, P, N, bake):
    """test_gpu_walkers' worlds, two ticks: slot 0 at 40 m/s - phase A's reach beyond the near lists, and where it slides a metre or more
    phase B's as well - slot 1 at 9 m/s, the rest in the short tier.  Of five envs the second is reset, the fourth has no walker and the
    third one walker far outside the plan, whom nothing blocks: that env leaves before phase B while its block's others go on."""
    sc, agents, walls, store, towards, dev = _world((plans(3) + plans(3, oblique=True))[:N], A, P, 7*A + P + 100*SEEDS[P, N], bake, fast={0: 40., 1: 9.})
    reset, hi = np.zeros(N, np.uint8), sc.WALL_GRID_REACH[1]
    if N == 5:
        store['positions'][3], reset[1] = NAN, 1
        store['positions'][2, 1:], store['positions'][2, 0] = NAN, walls[2].reshape(-1, 2).max(0) + 50
        towards[2, 0] = _dev(store['positions'][2, 0] + 1)
    slid = stopped = reach = 0
    for _ in range(2):
        free = wr.host_walk([np.zeros((0, 4), np.float32)]*N, _np(agents.positions), store, _np(towards), keep=.3, radius=1e-6, reset=reset)['velocities']
        before, (store, want) = store['positions'], _tick(sc, agents, walls, store, towards, dev, reset=reset, keep=.3)
        moved = np.linalg.norm(want['positions'] - (before + want['progress'][..., None]*free/10), axis=-1)      # x2 |u2|, no more than |u2|
        reach = max(reach, np.nanmax(np.where(want['slid'] > 0, 1.02*(1.0102*moved + 2.002*AGENT_RADIUS) + 1e-3, 0)))  # (wall_reach)
        slid, stopped = slid + (want['slid'] > 0).sum(), stopped + (want['stopped'] == 1).sum()
        assert N == 1 or (want['progress'][2, 0] == 1 and (want['stopped'][[1, 3]] == 4).all() and np.isnan(want['slid'][[1, 3]]).all())
    assert slid > 0 and stopped > 0 and reach > 1.05*hi


def test_eight_sliding_ticks_in_a_row_then_three_replays_of_a_graph():
    """Two plans, the store and the records compared after every tick; `out=` on a side stream; then three replays, each a later tick."""
    from megastep_amd import cuda
    sc, agents, walls, store, towards, dev = _world(plans(3)[1:], 3, 40, 11)
    kw, slide = dict(personal=.5, push=1.5, keep=.6), dict(bounce=.1)
    side, walked, slides = torch.cuda.Stream(), None, 0

    def eager():
        nonlocal walked
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            out = cuda.walk(sc, agents, dev, towards, out=walked, slide=slide, **kw)
        assert walked is None or out is walked
        walked = out
        return out

    for t in range(8):
        store, want = _tick(sc, agents, walls, store, towards, dev, load=t == 0, walk=eager, slide=slide, **kw)
        slides += (want['slid'] > 0).sum()
    with pytest.raises(RuntimeError, match='same shapes'):
        cuda.walk(sc, agents, dev, towards, out=walked, **kw)            # (a sliding walk's result is not a plain walk's)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cuda.walk(sc, agents, dev, towards, out=walked, slide=slide, **kw)
    for t in range(3):
        store, want = _tick(sc, agents, walls, store, towards, dev, load=False, walk=lambda: graph.replay() or walked, slide=slide, **kw)
        slides += (want['slid'] > 0).sum()
    assert slides > 0 and np.isfinite(store['positions']).all(-1).any()


@pytest.mark.parametrize('P', [64, 65])
def test_a_walk_without_slide_is_still_the_plain_host_statement(P):
    sc, agents, walls, store, towards, dev = _world(plans(3)[:2], 2, P, P, fast={0: 40.})
    _tick(sc, agents, walls, store, towards, dev, slide=False, keep=.3)
