"""The fan schedule (MsAgents.schedule) on the GPU: a render that starts its waves in the order the physics launch sorted last
frame's costs into computes, bit for bit, what a render in fan order computes - at the headline shape and at C2, through renders
without a physics step between them, physics steps without a render, a buffer full of garbage, and without a buffer."""
import numpy as np
import pytest
import torch

from tests import util
from tests.test_fan_order_host import assert_order_follows_the_rule, klass

pytestmark = pytest.mark.gpu

PLANES = ('indices', 'locations', 'dots', 'distances', 'screen')


def _world(n_envs, n_agents, seed=0):
    from megastep_amd import core, cubicasa, cuda, modules, scene
    np.random.seed(seed)
    torch.manual_seed(seed)
    pool = cubicasa.sample(256, split='all', n_unique=256, seed=seed + 1, workers=16, context='subprocess')
    geometries = [pool[i % len(pool)] for i in range(n_envs)]
    scenery = scene.scenery(geometries, n_agents, device='cuda', random=np.random.RandomState(seed), fast=True, bake=False)
    cuda.bake(scenery)
    c = core.Core(scenery, res=64, fov=130, fps=10)
    modules.RandomSpawns(geometries, c, fast=True)(c.agent_full(True))
    return c


def _tensors(c):
    a = c.agents
    return (a.angles, a.positions, a.angvelocity, a.velocity, c.scenery.lines.vals)


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _same(x, y):
    return torch.equal(_bits(x), _bits(y))


def _use(c, mode):
    """'off': the switch off; 'on' / 'garbage': the schedule followed; 'null': the agents carry none."""
    from megastep_amd import _lib
    _lib.lib().ms_debug_render_order(0 if mode == 'off' else 1)
    ptr = None if mode == 'null' else c.agents._schedule.data_ptr()
    c.agents._struct.schedule = ptr
    c.agents._plain.schedule = ptr


def _rollout(c, start, script, vels, mode, seed=11):
    """Plays `script` - per step a string of P (physics), R (render) - from `start`; every R's planes and lines, every P's progress
    and agent state, in order."""
    from megastep_amd import cuda
    for t, s in zip(_tensors(c), start):
        t.copy_(s)
    c.agents._headings.fill_(float('nan'))
    c.agents._cached = False
    c.agents._schedule[0].zero_()
    c.agents._schedule[1].copy_(torch.arange(c.agents._schedule.shape[1], dtype=torch.int32, device=c.device))
    _use(c, mode)
    gen = torch.Generator(device='cpu').manual_seed(seed)
    seen = []
    try:
        for ops, (v, w) in zip(script, vels):
            c.agents.velocity.copy_(v); c.agents.angvelocity.copy_(w)
            for op in ops:
                if op == 'P':
                    if mode == 'garbage':        # (anything at all, costs and order: the sort in front of the next render writes a permutation)
                        junk = torch.randint(-2**31, 2**31 - 1, tuple(c.agents._schedule.shape), generator=gen, dtype=torch.int64)
                        c.agents._schedule.copy_(junk.to(torch.int32))
                    p = cuda.physics(c.scenery, c.agents)
                    seen.append(('P', [p.progress.clone()] + [t.clone() for t in _tensors(c)[:4]]))
                else:
                    r = cuda.render(c.scenery, c.agents)
                    seen.append(('R', [getattr(r, f).clone() for f in PLANES] + [c.scenery.lines.vals.clone()]))
    finally:
        _use(c, 'on')
        from megastep_amd import _lib
        _lib.lib().ms_debug_render_order(1)
    return seen


def _assert_equal(ref, got, what):
    assert len(ref) == len(got)
    for i, ((ka, xa), (kb, xb)) in enumerate(zip(ref, got)):
        assert ka == kb
        for j, (x, y) in enumerate(zip(xa, xb)):
            assert _same(x, y), f'{what}: {"progress/state" if ka == "P" else "planes/lines"} tensor {j} differs at call {i} ({ka})'


def _check_order_on_device(c):
    """After a physics step: the order row is, class for class and share for share, the rule's for the costs row next to it
    (tests/test_fan_order_host.py, order_rule) - every slot written, every sort wave's share of the slots a permutation of its own
    fans, the classes' sequence the rule's."""
    costs, order = (t.cpu().numpy() for t in c.agents._schedule)
    assert_order_follows_the_rule(costs, order, what=f'{len(costs)} fans')
    return klass(costs)


@pytest.mark.parametrize('n_envs, n_agents', [(4096, 4), (4096, 1)], ids=['headline', 'c2'])
def test_the_order_changes_no_bit(n_envs, n_agents):
    c = _world(n_envs, n_agents)
    rng = np.random.RandomState(5)
    steps = 25
    vels = []
    for i in range(steps):
        util.random_velocities(c, rng, speed=3. if i % 3 else 12.)
        vels.append((c.agents.velocity.clone(), c.agents.angvelocity.clone()))
    start = [t.clone() for t in _tensors(c)]
    plain = steps*['PR']
    # ... two renders without a physics step between them, two physics steps without a render
    mixed = [('PRR' if i % 5 == 1 else 'PPR' if i % 5 == 3 else 'PR') for i in range(steps)]
    ref_plain = _rollout(c, start, plain, vels, 'off')
    _assert_equal(ref_plain, _rollout(c, start, plain, vels, 'on'), 'order on')
    cls = _check_order_on_device_after_a_step(c)
    if n_agents > 1:
        assert len(np.unique(cls)) > 3, 'the waves report different costs'
    progress = torch.stack([x[0] for k, x in ref_plain if k == 'P'])
    assert (progress < 1).any() and (progress == 1).any()
    ref_mixed = _rollout(c, start, mixed, vels, 'off')
    _assert_equal(ref_mixed, _rollout(c, start, mixed, vels, 'on'), 'order on, renders and steps doubled')
    _assert_equal(ref_mixed, _rollout(c, start, mixed, vels, 'garbage'), 'garbage in the buffer')
    _assert_equal(ref_mixed, _rollout(c, start, mixed, vels, 'null'), 'no buffer')


def _check_order_on_device_after_a_step(c):
    from megastep_amd import cuda
    c.agents._schedule[1].fill_(-12345)          # (no slot may keep it)
    cuda.physics(c.scenery, c.agents)            # (sorts what the last render left)
    torch.cuda.synchronize()
    return _check_order_on_device(c)
