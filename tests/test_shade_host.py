"""Shading of given rays (`ms_shade` / `cuda.shade`, `ms_camera_pose_rays` / `cuda.cameras`) on the CPU: the numpy statement of
the rule (tests/shade_rule.py) is the oracle's render, bit for bit, on the rays the oracle can cast; `ms_host_shade` - the
serial host statement over the kernel's own per-ray functions - is the numpy statement, bit for bit, on those worlds and on
hand-made ones; the C-ABI declares, binds and checks the new calls."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import shade_rule as S
from tests.test_abi import ROOT, declared_symbols

F = np.float32
NEW = ('ms_shade', 'ms_camera_pose_rays')


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.int32)


# ---- the rays the oracle can cast: two plans, three agents in sight of each other -------------------------------------------------
@pytest.fixture(scope='module')
def plans(oracle):
    """(scene dict with the oracle's baked light, agents dict, the oracle's render, its drawn lines), res 64 and 37."""
    from tests import util
    out = []
    for res, seed in ((64, 21), (37, 22)):
        c = S.triangle_world(2, res, seed, 'cpu')            # a triangle of agents looking at each other
        ref = util.OracleWorld(c)
        ref.bake()
        want = ref.render()                                # (draws the agents' rows into ref.scene.lines_vals)
        scene = util.scene_dict(c.scenery)
        scene['baked_vals'] = ref.scene.baked_vals.copy()
        out.append((scene, ref.agents, want, ref.scene.lines_vals.copy()))
    return out


def _flat(want, k):
    n, a, r = want['indices'].shape
    return want[k].reshape(n, a*r, *want[k].shape[3:])


def test_the_numpy_rule_is_the_oracles_screen(plans):
    """shade_rule fed with the oracle's own indices, locations, dots and drawn lines: the oracle's `screen`, as bits - with rays
    that landed on an agent among them - and the rows it would draw itself are the oracle's."""
    for scene, agents, want, drawn in plans:
        AF = scene['n_agents']*len(scene['model'])
        idx = _flat(want, 'indices')
        assert ((idx >= 0) & (idx < AF)).sum() > 0 and (idx >= AF).sum() > 0
        got = S.shade_rule(scene, drawn, idx, _flat(want, 'locations'), _flat(want, 'dots'))
        np.testing.assert_array_equal(_bits(got), _bits(_flat(want, 'screen')))
        np.testing.assert_array_equal(_bits(S.draw_rows(scene, agents)), _bits(drawn))
        assert (got[(idx >= 0) & (idx < AF)] > 0).any()                        # (the bodies are lit, not black)


def test_the_host_statement_is_the_rule_on_the_plans(plans):
    for scene, agents, want, drawn in plans:
        planes = [_flat(want, k) for k in ('indices', 'locations', 'dots')]
        got = S.host_shade(scene, agents, *planes)
        np.testing.assert_array_equal(_bits(got), _bits(_flat(want, 'screen')))
        bare = S.host_shade(scene, None, *planes)
        np.testing.assert_array_equal(_bits(bare), _bits(S.shade_rule(scene, drawn, *planes, with_agents=False)))
        AF = scene['n_agents']*len(scene['model'])
        on_body = (planes[0] >= 0) & (planes[0] < AF)
        assert not bare[on_body].any() and np.array_equal(_bits(bare[~on_body]), _bits(got[~on_body]))


def test_the_gpu_tests_plan_worlds_have_rays_on_agents(oracle):
    """The seeds of tests/test_gpu_cameras.py's plan worlds, checked here with the oracle: rays land on an agent in each."""
    from tests import util
    for n_envs, res, seed in S.LOOK_WORLDS:
        c = S.triangle_world(n_envs, res, seed, 'cpu')
        idx = util.OracleWorld(c).render()['indices']
        assert ((idx >= 0) & (idx < 3*len(c.scenery.model))).sum() > 20


# ---- hand-made worlds ------------------------------------------------------------------------------------------------------------------
BOX = np.array([[[1, 1], [6, 1]], [[6, 1], [6, 6]], [[6, 6], [1, 6]], [[1, 6], [1, 1]]], float)
MODEL = np.array([[[-.125, 0.], [.125, 0.]], [[0., -.1], [.1, .1]], [[.1, .1], [-.1, .1]]], F)     # a bar and two sides


def hand_world(rng):
    """Five envs of two agents: a box with pillars, a light of intensity 0 and a line of texture width 1; a dark box; a box
    under 65 lights; three walls that meet in one vertex, the middle one through it, between a light and the first agent's bar;
    a single wall.  Returns (scene, agents)."""
    pillars = np.concatenate([np.array([[[x, y], [x + .3, y]], [[x + .3, y], [x + .3, y + .3]], [[x + .3, y + .3], [x, y + .3]],
                                        [[x, y + .3], [x, y]]]) for x, y in rng.uniform(1.5, 5., (5, 2))])
    AF = 2*len(MODEL)
    widths0 = rng.randint(1, 9, AF + 4 + len(pillars))
    widths0[[0, AF, AF + 5]] = 1                                               # an agent row, a wall and a pillar side of one texel
    vertex = np.array([[[2, 3], [3, 3]], [[3, 3], [4, 3]], [[3, 2.5], [3, 3.5]]], float)
    envs = [
        dict(walls=np.concatenate([BOX, pillars]), lights=[[2., 2., 1.], [5., 5., 0.], [3.5, 4.5, .4]], widths=widths0),
        dict(walls=BOX, lights=np.zeros((0, 3))),
        dict(walls=np.concatenate([BOX, pillars]), lights=np.concatenate([rng.uniform(1.2, 5.8, (65, 2)), rng.uniform(.002, .03, (65, 1))], 1)),
        dict(walls=np.concatenate([BOX, vertex]), lights=[[3., 1.5, .5], [1.5, 4., .2]]),
        dict(walls=BOX[:1], lights=[[3., 3., 1.]]),
    ]
    scene = S.make_scene(2, MODEL, envs, rng)
    positions = rng.uniform(1.5, 5.5, (5, 2, 2)).astype(F)
    angles = rng.uniform(-180, 180, (5, 2)).astype(F)
    positions[3, 0], angles[3, 0] = (3., 5.), 90.          # the bar at x = 3 exactly, end on to the light: the sight line runs through the vertex
    return scene, dict(angles=angles, positions=positions)


def hand_rays(scene, R, rng):
    """(N, R) planes: indices from -1 (a miss) to the env's line count (no line: black), agent rows as likely as walls; locations
    in [0, 1], exactly 0 and exactly 1 among them; dots in [-1, 1]."""
    lw = np.asarray(scene['lines_widths'])
    AF = scene['n_agents']*len(scene['model'])
    N = len(lw)
    idx = np.stack([np.where(rng.rand(R) < .5, rng.randint(0, AF, R), rng.randint(-1, lw[n] + 1, R)) for n in range(N)]).astype(np.int32)
    loc = rng.uniform(0, 1, (N, R)).astype(F)
    loc[rng.rand(N, R) < .1] = 0.
    loc[rng.rand(N, R) < .1] = 1.
    dots = rng.uniform(-1, 1, (N, R)).astype(F)
    # ... and, whatever was drawn: a miss, the line count, the first agent's bar at its middle and its ends
    idx[:, 0], loc[:, 0] = 0, .5
    if R > 1:
        idx[:, 1], idx[:, 2], idx[:, 3], idx[:, 4] = -1, lw, 0, 0
        loc[:, 3], loc[:, 4] = 0., 1.
    return idx, loc, dots


@pytest.mark.parametrize('R', [1, 37, 64])
def test_the_host_statement_is_the_rule_on_hand_made_worlds(oracle, R):
    rng = np.random.RandomState(100 + R)
    scene, agents = hand_world(rng)
    idx, loc, dots = hand_rays(scene, R, rng)
    drawn = S.draw_rows(scene, agents)
    want = S.shade_rule(scene, drawn, idx, loc, dots)
    got = S.host_shade(scene, agents, idx, loc, dots)
    np.testing.assert_array_equal(_bits(got), _bits(want))
    AF = 2*len(MODEL)
    lw = np.asarray(scene['lines_widths'])[:, None]
    black = (idx < 0) | (idx >= lw)
    assert not got[black].any()                                                # misses and indices that are no line: (0, 0, 0)
    assert (got[3, 0] > 0).all()                                               # through the shared vertex the light arrives
    assert got[1][(idx[1] >= 0) & (idx[1] < AF)].max(initial=0) <= F(.1001)      # a dark env: ambient light alone on a body
    bare = S.host_shade(scene, None, idx, loc, dots)
    np.testing.assert_array_equal(_bits(bare), _bits(S.shade_rule(scene, drawn, idx, loc, dots, with_agents=False)))
    assert not bare[(idx >= 0) & (idx < AF)].any()                             # agent rows without agents: black
    np.testing.assert_array_equal(_bits(bare[idx >= AF]), _bits(got[idx >= AF]))


def test_the_vertex_case_is_what_it_says(oracle):
    """In env 3 the sight line from the first light to the middle of the first agent's bar passes through the vertex three walls
    share: t is exactly 1 on one, exactly 0 on the next, the third is parallel - none blocks (kernels.cu:238-259), while a
    point a little to the side is in shadow of the middle wall's neighbours."""
    rng = np.random.RandomState(7)
    scene, agents = hand_world(rng)
    drawn = S.draw_rows(scene, agents)
    ls = S.starts_of(scene['lines_widths'])
    (ax, ay), (bx, by) = drawn[ls[3]]
    assert ax == bx == F(3) and ay != by
    AF = 2*len(MODEL)
    walls = drawn[ls[3] + AF:ls[3] + scene['lines_widths'][3]]
    lights = np.asarray(scene['lights_vals']).reshape(-1, 3)[S.starts_of(scene['lights_widths'])[3]:][:1]
    through = S.light_intensity((F(3), F(5)), lights, walls)
    beside = S.light_intensity((F(3.2), F(5)), lights, walls)
    assert through > S.AMBIENT and beside == S.AMBIENT


# ---- the C-ABI -----------------------------------------------------------------------------------------------------------------------
def test_the_headers_declare_the_new_calls_and_the_library_exports_them():
    from megastep_amd import _lib
    assert set(NEW) <= set(declared_symbols(('megastep_hip.h',)))
    assert 'ms_host_shade' in declared_symbols(('megastep_hip_test.h',)) and 'ms_host_shade' not in declared_symbols(('megastep_hip.h',))
    assert set(NEW) | {'ms_host_shade'} <= set(_lib.SYMBOLS)
    text = open(os.path.join(ROOT, 'include', 'megastep_hip.h')).read()
    assert int(re.search(r'#define MS_ABI_VERSION (\d+)', text).group(1)) == _lib.ABI_VERSION == 17
    handle = _lib.lib()
    for name in NEW + ('ms_host_shade',):
        assert hasattr(handle, name), name
    assert handle.ms_abi_version() == 17


def test_the_new_calls_reject_bad_arguments_before_any_launch(oracle):
    from megastep_amd import _lib
    h = _lib.lib()
    assert h.ms_shade(None, None, None, None, None) == -1
    assert h.ms_shade(ctypes.byref(_lib.MsScenery()), None, ctypes.byref(_lib.MsShade()), None, None) == -1
    assert h.ms_camera_pose_rays(None, None) == -1
    assert h.ms_camera_pose_rays(ctypes.byref(_lib.MsCameraPoses()), None) == -1
    assert h.ms_host_shade(None, None, None) == -1
    rng = np.random.RandomState(0)
    scene, agents = hand_world(rng)
    sc, ag, keep = S.host_structs(scene, agents)
    idx, loc, dots = (S._aligned(a, t) for a, t in zip(hand_rays(scene, 8, rng), (np.int32, F, F)))
    screen = S._aligned(np.zeros((5, 8, 3)), F)
    p = lambda a: a.ctypes.data
    good = lambda: _lib.MsShade(8, p(idx), p(loc), p(dots), p(screen))
    assert h.ms_host_shade(ctypes.byref(sc), ctypes.byref(ag), ctypes.byref(good())) == 0
    for field, value in (('n_rays', 0), ('indices', None), ('locations', None), ('dots', None), ('screen', None), ('dots', p(dots) + 2)):
        q = good()
        setattr(q, field, value)
        assert h.ms_host_shade(ctypes.byref(sc), ctypes.byref(ag), ctypes.byref(q)) == -1, field
        assert h.ms_shade(ctypes.byref(sc), ctypes.byref(ag), ctypes.byref(q), None, None) == -1, field
    no_poses = _lib.MsAgents(None, None, None, None, None, None)
    assert h.ms_host_shade(ctypes.byref(sc), ctypes.byref(no_poses), ctypes.byref(good())) == -1
    assert h.ms_shade(ctypes.byref(sc), ctypes.byref(no_poses), ctypes.byref(good()), None, None) == -1
    # a light grid that is not usable: verdicts without their geometry, or off their alignment
    sc.lg_vals = p(keep['lines'])
    assert h.ms_shade(ctypes.byref(sc), ctypes.byref(ag), ctypes.byref(good()), None, None) == -1
    sc.lg_starts, sc.lg_geom, sc.lg_cell = p(keep['ls']), p(keep['lines']), .125
    sc.lg_vals = p(keep['lines']) + 4
    assert h.ms_shade(ctypes.byref(sc), ctypes.byref(ag), ctypes.byref(good()), None, None) == -1
    # cameras: fields of view outside a projection's range, no rays, a projection that is none
    buf = S._aligned(np.zeros((2, 16, 2)), F)
    poses = S._aligned(np.zeros((2, 2, 3)), F)
    for res, fov, proj in ((0, 90., 0), (8, 0., 0), (8, 180., 0), (8, 361., 1), (8, float('nan'), 1), (8, 90., 2)):
        cams = _lib.MsCameraPoses(2, 2, res, p(poses), fov, proj, p(buf), p(buf))
        assert h.ms_camera_pose_rays(ctypes.byref(cams), None) == -1, (res, fov, proj)
    cams = _lib.MsCameraPoses(2, 2, 8, p(poses), 90., 0, p(buf) + 4, p(buf))
    assert h.ms_camera_pose_rays(ctypes.byref(cams), None) == -1


def test_the_python_layer_refuses_what_it_cannot_run():
    from megastep_amd import cuda
    from tests import util
    c, _ = util.plan_world(2, 2, 16, 90, seed=1, device='cpu')
    hits = cuda.Raycast(torch.zeros(2, 5, dtype=torch.int32), torch.zeros(2, 5), torch.zeros(2, 5), None, None)
    with pytest.raises(RuntimeError, match='GPU'):
        cuda.shade(c.scenery, hits)
    with pytest.raises(RuntimeError, match='indices, locations and dots'):
        cuda.shade(c.scenery, cuda.Raycast(hits.indices, None, hits.dots, None, None))
    with pytest.raises(RuntimeError, match='n_envs'):
        cuda.shade(c.scenery, cuda.Raycast(torch.zeros(3, 5, dtype=torch.int32), torch.zeros(3, 5), torch.zeros(3, 5), None, None))
    with pytest.raises(RuntimeError, match='GPU'):
        cuda.cameras(torch.zeros(2, 1, 3), 8, 90)
    with pytest.raises(RuntimeError, match='cams'):
        cuda.look(c.scenery, None)
    assert cuda.RAYCAST_FIELDS == ('indices', 'locations', 'dots', 'distances', 'agents')
    assert cuda.LOOK_FIELDS == ('screen',) + cuda.RAYCAST_FIELDS
