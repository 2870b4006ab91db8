"""Records the reference's own kernels on a fixed list of small cases -> tests/golden/reference_kernels.npz.

Run from the repository root, where oracle/_ref holds the reference built for the host (oracle/reference.py):

    python tests/golden/make_reference_kernels.py

Arrays only. Each case is stored with its FULL INPUTS - scene arrays, config, agents - not with the seeds its builder drew
them from, so that a change to a generator cannot quietly change a stored case; and with what the reference made of them:
the baked light, one physics step (progress, the four agent tensors after it) and the render from the state that step left
(indices, locations, dots, distances, screen). tests/test_gpu_reference_pin.py reads nothing else.

At most 6 envs, 4 agents and 128 rays a case; floorplans are cut down to the room round the agents (util.crop_case)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle import reference           # noqa: E402
from tests import util                 # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'reference_kernels.npz')
SCENE_ARRAYS = ('model', 'lights_vals', 'lights_widths', 'lines_vals', 'lines_widths', 'textures_vals', 'textures_widths')


def _with_move(case, step):
    """The case with the velocities of one of its moves set on its agents (what the one recorded step uses)."""
    velocity, angvelocity = case['moves'][step]
    return dict(case, agents=dict(case['agents'], velocity=velocity.copy(), angvelocity=angvelocity.copy()))


def _plan(n_envs, n_agents, res, fov, seed, speed, oblique=False, radius=2.5):
    if oblique:
        c, _ = util.oblique_world(n_envs, n_agents, res, fov, False, device='cpu')
    else:
        c, _ = util.plan_world(n_envs, n_agents, res, fov, seed=seed, device='cpu')
    if n_agents > 1:                                                    # someone to look at (and to run into), in the first env
        c.agents.positions[0, 1] = c.agents.positions[0, 0] + c.agents.positions.new_tensor([.4, .1])
    moves = util.random_moves((n_envs, n_agents), np.random.RandomState(seed + 20), (speed,))
    return crop_case_checked(util.case_of(c, moves), radius)


def crop_case_checked(case, radius):
    cropped = util.crop_case(case, radius)
    assert (cropped['scene']['lines_widths'] > 8*cropped['scene']['n_agents'] + 3).all(), 'a room has walls'
    return cropped


def cases():
    rng = np.random.RandomState(0)
    box, _ = util.plan_world(2, 2, 64, 130, toy='box', device='cpu')
    column, _ = util.plan_world(2, 2, 64, 70, toy='column', device='cpu')
    meeting = util.case_of(util.agents_meeting_agents_world(4, device='cpu'), [])
    crawling = util.case_of(util.crawling_agents_world(device='cpu'), [])
    broken = util.case_of(util.non_finite_walls_world(4, device='cpu'), [])
    lights = util.case_of(util.many_lights_world(util.many_lights_geometries(rng), rng, device='cpu'), [])
    ragged = util.ragged_edge_world(np.random.RandomState(0), device='cpu', many_walls=False)
    hysteresis = util.case_of(util.hysteresis_band_world(device='cpu'), [])
    wedged = util.case_of(util.wedged_agent_world(device='cpu'), [])
    endpoint, parallel, grazing = util.endpoint_case(), util.near_parallel_case(), util.grazing_light_case()
    standing = lambda case: dict(case, moves=util.still(case))
    return {
        'box': util.case_of(box, util.random_moves((2, 2), np.random.RandomState(7), (40.,))),
        'column': util.case_of(column, util.random_moves((2, 2), np.random.RandomState(7), (4.,))),
        'plan_a': _plan(2, 4, 64, 130, seed=0, speed=40.),
        'plan_b': _plan(2, 1, 64, 90, seed=3, speed=6., radius=2.),
        'oblique_a': _plan(2, 3, 100, 130, seed=0, speed=40., oblique=True),
        'oblique_b': _plan(2, 1, 128, 160, seed=5, speed=6., oblique=True, radius=2.),
        'hysteresis_band': util.take_envs(standing(hysteresis), [0, 3, 4, 8, 12, 21]),
        'coincident_walls': standing(wedged),
        'agents_meet_agents': util.take_envs(standing(meeting), [0, 5, 11]),      # in step, NaN and inf states among them
        'crawling_agents': util.take_envs(standing(crawling), [0, 1, 2]),
        'non_finite_walls': util.take_envs(standing(broken), [1, 2, 5]),
        'many_lights': standing(lights),                                                       # 70, 9, 150 and 64 lights: past the light grid's 64 an env, and at it
        'ragged_edges': util.case_of(ragged, util.random_moves((3, 2), np.random.RandomState(1), (5.,))),
        'wall_endpoints': util.take_envs(dict(endpoint, moves=endpoint['moves'][:1]), [0, 7, 14, 21, 42, 63]),
        'shared_corners': util.crop_case(util.take_envs(util.corner_fan_case()[1], [0, 2]), 2.1),
        'near_parallel': util.take_envs(dict(parallel, moves=parallel['moves'][:1]), [4, 6, 8, 10, 13, 15]),
        'grazing_light': util.take_envs(grazing, [6, 10, 12, 13, 14, 18]),
        'narrow_textures': util.narrow_textures_case(),
    }


def record(case):
    case = _with_move(case, 0)
    scene, config, agents = case['scene'], case['config'], case['agents']
    N, A = agents['angles'].shape
    assert N <= 6 and A <= 4 and config[1] <= 128, (N, A, config)
    world = reference.World(scene, config)
    out = {'scene_' + k: np.asarray(scene[k]) for k in SCENE_ARRAYS}
    out.update(n_agents=np.asarray(scene['n_agents'], np.int32), config=np.asarray(config, np.float64))
    out.update({'agents_' + k: v for k, v in agents.items()})
    out['baked'] = world.bake()
    out['progress'], after = world.physics(agents)
    out.update({'after_' + k: v for k, v in after.items()})
    out.update(world.render(after))
    return {k: np.asarray(v) for k, v in out.items()}


def main():
    records = {}
    for name, case in cases().items():
        rec = records[name] = record(case)
        print(f"{name:20s} envs {len(rec['scene_lines_widths'])} agents {int(rec['n_agents'])} rays {int(rec['config'][1]):4d} "
              f"lines {len(rec['scene_lines_vals']):5d} texels {len(rec['scene_textures_vals']):6d} "
              f"collisions {int((rec['progress'] < 1).sum())} hits {int((rec['indices'] >= 0).sum())}/{rec['indices'].size} "
              f"on agents {int(((rec['indices'] >= 0) & (rec['indices'] < 8*int(rec['n_agents']))).sum())}")
    arrays = util.pack_cases(records)
    np.savez_compressed(OUT, **arrays)
    back = util.load_cases(OUT)
    assert list(back) == list(records) and all(np.array_equal(back[n][k], v, equal_nan=v.dtype.kind == 'f') and back[n][k].dtype == v.dtype
                                              for n, rec in records.items() for k, v in rec.items())
    print(f'{OUT}: {os.path.getsize(OUT)/1e3:.0f} kB, {len(arrays)} arrays')


if __name__ == '__main__':
    main()
