"""Ray queries (`ms_raycast` / `cuda.raycast`, `ms_camera_rays` / `cuda.camera_rays`) on the CPU: the C-ABI declares and binds
them, the Python layer refuses what it cannot cast, and the numpy rule the GPU tests (tests/test_gpu_raycast.py) hold the kernel
to is checked here against the oracle's render on the rays the oracle can express - its camera rays."""
import ctypes
import ctypes.util
import os
import re

import numpy as np
import pytest
import torch

from tests.test_abi import ROOT, declared_symbols

F = np.float32


def raycast_rule(lines, origins, dirs, near):
    """The reference's per-ray rule, kernels.cu:349-382, restated in binary32 numpy (every operation rounded to float32, as
    the reference compiles it): over `lines` (L, 2, 2) in line order, for rays from `origins` (R, 2) along `dirs` (R, 2) -
    intersect() of kernels.cu:67-89 (s, t from two cross products over cross(ru, v), no hit when |cross(ru, v)| < 1e-3); a hit
    when 0 <= t <= 1, better when near/|ru| < s < nearest - 1e-4 (kernels.cu:366-370); dot(ru, v)/(|ru||v| + 1e-6)
    (kernels.cu:360-364); distance = nearest*|ru| (kernels.cu:382).  Returns indices, locations, dots, distances."""
    lines = np.asarray(lines, F).reshape(-1, 2, 2)
    px, py = np.asarray(origins, F)[:, 0], np.asarray(origins, F)[:, 1]
    ux, uy = np.asarray(dirs, F)[:, 0], np.asarray(dirs, F)[:, 1]
    R = len(px)
    rlen = np.sqrt(ux*ux + uy*uy)
    near_s = F(near)/rlen
    best = np.full(R, np.inf, F)
    idx = np.full(R, -1, np.int32)
    loc = np.full(R, np.nan, F)
    dt = np.full(R, np.nan, F)
    with np.errstate(all='ignore'):
        for l, ((ax, ay), (bx, by)) in enumerate(lines):
            vx, vy = F(bx - ax), F(by - ay)
            uxv = ux*vy - uy*vx                                  # cross(U, V)
            pqx, pqy = F(ax) - px, F(ay) - py                    # PQ = Q - P
            parallel = np.abs(uxv) < F(1e-3)
            s = np.where(parallel, F(np.inf), (pqx*vy - pqy*vx)/uxv)
            t = np.where(parallel, F(np.inf), (pqx*uy - pqy*ux)/uxv)
            dot = (ux*vx + uy*vy)/(rlen*np.sqrt(vx*vx + vy*vy) + F(1e-6))
            take = (F(0) <= t) & (t <= F(1)) & (near_s < s) & (s < best - F(1e-4))
            best = np.where(take, s, best)
            idx = np.where(take, np.int32(l), idx)
            loc = np.where(take, t, loc)
            dt = np.where(take, dot, dt)
        dist = best*rlen
    return dict(indices=idx, locations=loc, dots=dt, distances=dist)


def camera_rays_np(angles, res, fov):
    """ru of every camera ray, (N, A, res, 2), as the oracle forms them: sincospi of angle/180 (the oracle's own), ray_y with
    the C library's tanf for the half-screen width (kernels.cu:22,234-236,334-337)."""
    from oracle import oracle as O
    libm = ctypes.CDLL(ctypes.util.find_library('m'))
    libm.tanf.restype, libm.tanf.argtypes = ctypes.c_float, [ctypes.c_float]
    arg = F(F(F(3.14159265358979323846)/F(180))*F(fov))/F(2)
    hs = F(libm.tanf(arg))
    Rf = F(res)
    r = np.arange(res).astype(F)
    yray = (Rf - F(2)*r - F(1))*hs/Rf
    angles = np.asarray(angles, F)
    out = np.zeros(angles.shape + (res, 2), F)
    for i in np.ndindex(angles.shape):
        s, c = O.sincospi(F(angles[i]/F(180)))
        out[i + (slice(None), 0)] = c*F(1) - s*yray
        out[i + (slice(None), 1)] = s*F(1) + c*yray
    return out


def test_the_header_declares_both_queries_and_the_loader_binds_them():
    from megastep_amd import _lib
    public = declared_symbols(('megastep_hip.h',))
    assert {'ms_raycast', 'ms_camera_rays'} <= set(public)
    assert {'ms_raycast', 'ms_camera_rays'} <= set(_lib.SYMBOLS)
    text = open(os.path.join(ROOT, 'include', 'megastep_hip.h')).read()
    assert int(re.search(r'#define MS_ABI_VERSION (\d+)', text).group(1)) == _lib.ABI_VERSION == 17
    handle = _lib.lib()
    assert hasattr(handle, 'ms_raycast') and hasattr(handle, 'ms_camera_rays')
    assert handle.ms_abi_version() == 17


def test_msraycast_mirror_has_the_c_layout():
    import subprocess
    import tempfile
    from megastep_amd import _lib
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "megastep_hip.h"\n'
           'int main(){printf("%zu %zu %zu", sizeof(MsRaycast), offsetof(MsRaycast, near_plane), offsetof(MsRaycast, grid_rays));}')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, 't.c'), 'w').write(src)
        subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), os.path.join(d, 't.c'), '-o', os.path.join(d, 't')])
        sizes = list(map(int, subprocess.check_output([os.path.join(d, 't')]).split()))
    assert sizes == [ctypes.sizeof(_lib.MsRaycast), _lib.MsRaycast.near_plane.offset, _lib.MsRaycast.grid_rays.offset]


def test_the_entry_points_reject_bad_arguments_before_any_launch():
    from megastep_amd import _lib
    h = _lib.lib()
    cfg = _lib.MsConfig(.1, 64, 130., 10.)
    q = _lib.MsRaycast(8, None, None, .1, None, None, None, None, None, None)
    assert h.ms_raycast(None, None, ctypes.byref(q), ctypes.byref(cfg), None) == -1
    assert h.ms_raycast(None, None, None, None, None) == -1
    ag = _lib.MsAgents(None, None, None, None, None)
    assert h.ms_camera_rays(ctypes.byref(ag), 1, 1, ctypes.byref(cfg), None, None) == -1
    assert h.ms_camera_rays(None, 1, 1, ctypes.byref(cfg), None, None) == -1


def _cpu_world(n_envs=2, n_agents=2):
    from megastep_amd import core, cubicasa, scene
    from tests import util
    np.random.seed(0)
    geoms = cubicasa.sample(n_envs, n_unique=16)
    sc = scene.scenery(geoms, n_agents, device='cpu', random=np.random.RandomState(0), bake=False)
    c = core.Core(sc, res=16, fov=90)
    util.spawn(c, geoms, seed=1)
    return c


def test_raycast_and_camera_rays_refuse_cpu_tensors_and_mismatched_shapes():
    from megastep_amd import cuda
    c = _cpu_world()
    n = len(c.scenery.lines)
    o, d = torch.zeros(n, 5, 2), torch.ones(n, 5, 2)
    with pytest.raises(RuntimeError, match='GPU'):
        cuda.raycast(c.scenery, o, d, near=.1)
    with pytest.raises(RuntimeError, match='GPU'):
        cuda.raycast(c.scenery, o, d, agents=c.agents)
    with pytest.raises(RuntimeError, match='GPU'):
        cuda.camera_rays(c.agents)
    with pytest.raises(RuntimeError, match='origins and directions'):
        cuda.raycast(c.scenery, o, torch.ones(n, 4, 2), near=.1)            # R differs
    with pytest.raises(RuntimeError, match='origins and directions'):
        cuda.raycast(c.scenery, torch.zeros(n, 5, 3), torch.ones(n, 5, 3), near=.1)
    with pytest.raises(RuntimeError, match='n_envs'):
        cuda.raycast(c.scenery, torch.zeros(n + 1, 5, 2), torch.ones(n + 1, 5, 2), near=.1)   # N vs the scenery
    with pytest.raises(RuntimeError, match='dtype'):
        cuda.raycast(c.scenery, o.double(), d.double(), near=.1)
    with pytest.raises(RuntimeError, match='fields'):
        cuda.raycast(c.scenery, o, d, near=.1, fields=('screen',))


@pytest.mark.parametrize('n_agents,res,fov', [(1, 64, 130), (3, 100, 70), (2, 128, 90)])
def test_the_numpy_rule_is_the_oracles_render_on_camera_rays(n_agents, res, fov):
    """Camera rays from the agents' positions through raycast_rule over the lines the oracle's render drew: the oracle's
    indices, locations, dots and distances, bit for bit."""
    from megastep_amd import core, cubicasa, scene
    from tests import util
    np.random.seed(3)
    geoms = cubicasa.sample(3, n_unique=16)
    sc = scene.scenery(geoms, n_agents, device='cpu', random=np.random.RandomState(1), bake=False)
    c = core.Core(sc, res=res, fov=fov)
    util.spawn(c, geoms, seed=4)
    if n_agents > 1:                                       # two agents face to face so that rays land on an agent
        c.agents.positions[0, 1] = c.agents.positions[0, 0] + torch.tensor([.6, 0.])
        c.agents.angles[0, 0], c.agents.angles[0, 1] = 0., 180.
    ref = util.OracleWorld(c)
    want = ref.render()                                    # (draws the agents' rows into ref.scene.lines_vals)
    lines = ref.scene.lines_vals
    starts = np.concatenate([[0], np.cumsum(ref.scene.lines_widths)])
    dirs = camera_rays_np(ref.agents['angles'], res, fov)
    agent_hits = 0
    for n in range(len(geoms)):
        for a in range(n_agents):
            p = np.broadcast_to(ref.agents['positions'][n, a], (res, 2))
            got = raycast_rule(lines[starts[n]:starts[n + 1]], p, dirs[n, a], c.agent_radius)
            for k in ('indices', 'locations', 'dots', 'distances'):
                np.testing.assert_array_equal(got[k].view(np.int32), want[k][n, a].view(np.int32), err_msg=(n, a, k))
            agent_hits += int(((got['indices'] >= 0) & (got['indices'] < n_agents*len(sc.model))).sum())
    assert (want['indices'] >= 0).mean() > .5
    if n_agents > 1:
        assert agent_hits > 0
