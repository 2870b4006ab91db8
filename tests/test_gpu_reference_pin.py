"""The HIP kernels against the reference's own kernels, from recorded cases alone.

tests/golden/reference_kernels.npz holds, for a fixed list of small cases, the full inputs (scene arrays, config, agents) and
what the reference's kernels - compiled for the host, oracle/reference.py - made of them: the baked light, one physics step
and the render from the state it left (tests/golden/make_reference_kernels.py). Here cuda.bake / cuda.physics / cuda.render
(and cuda.step_render where it is one launch: one agent, at most 64 rays) run on the stored inputs, with the wall grid and
the light grid on and off, and are held to the stored outputs bit for bit (tests/util.py: assert_bits - any NaN equals any NaN):
collision masks, hit indices, every float of the agents' state and of the four render planes (also where a ray missed), the bake.

Neither the oracle nor the reference is touched: only the npz."""
import os

import numpy as np
import pytest
import torch

from tests import util

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'reference_kernels.npz')
CASES = util.load_cases(GOLDEN)
AGENT_FIELDS = ('angles', 'positions', 'angvelocity', 'velocity')
PLANES = ('indices', 'locations', 'dots', 'distances', 'screen')


def _world(g, wall_grid):
    """A baked cuda.Scenery and a Core over a stored case's inputs."""
    from megastep_amd import core, cuda
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device='cuda')
    scenery = cuda.Scenery(
        n_agents=int(g['n_agents']),
        lights=cuda.Ragged2D(t(g['scene_lights_vals']), t(g['scene_lights_widths'])),
        lines=cuda.Ragged3D(t(g['scene_lines_vals']), t(g['scene_lines_widths'])),
        textures=cuda.Ragged2D(t(g['scene_textures_vals']), t(g['scene_textures_widths'])),
        model=t(g['scene_model']))
    cuda.bake(scenery, wall_grid=wall_grid)
    radius, res, fov, fps = g['config']
    assert abs(radius - core.AGENT_RADIUS) < 1e-9, 'a Core has one agent radius'
    return core.Core(scenery, res=int(res), fov=float(fov), fps=float(fps))


def _place(c, g):
    for k in AGENT_FIELDS:
        getattr(c.agents, k)[:] = torch.as_tensor(g['agents_' + k], device=c.device)


@pytest.mark.parametrize('light_grid', [True, False], ids=['lightgrid', 'nolightgrid'])
@pytest.mark.parametrize('wall_grid', [True, False], ids=['wallgrid', 'nowallgrid'])
@pytest.mark.parametrize('name', list(CASES))
def test_kernels_give_what_the_references_kernels_gave(monkeypatch, name, wall_grid, light_grid):
    from megastep_amd import cuda
    monkeypatch.setattr(cuda.Scenery, 'LIGHT_GRID', light_grid)
    g = CASES[name]
    c = _world(g, wall_grid)
    assert wall_grid or c.scenery._wg is None
    after = {k: g['after_' + k] for k in AGENT_FIELDS}
    ref = {k: g[k] for k in PLANES}

    util.assert_bits(c.scenery.baked.vals, g['baked'], 'baked')

    _place(c, g)
    p = cuda.physics(c.scenery, c.agents)
    r = cuda.render(c.scenery, c.agents)
    util.assert_physics_bits(c, p, g['progress'], after)
    util.assert_render_bits(c, r, ref)

    if c.n_agents == 1 and c.res <= 64:             # the shape where a step is one launch
        _place(c, g)
        p, r = cuda.step_render(c.scenery, c.agents)
        util.assert_physics_bits(c, p, g['progress'], after)
        util.assert_render_bits(c, r, ref)
